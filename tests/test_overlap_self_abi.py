"""The self-intersection query's C-ABI surface (include/wgt_api.h: wgt_overlap_self and its forms): declared,
exported, bound, the struct's layout against the header, every refusal of check_overlap_self_args in the
header's order with its message, the refusals that need no scene, and plan_overlap_self's LDS bytes with its
refusal (through a small C++ program built against the planning layer).  No compute on a device (no GPU
needed).

The header writes these four declarations with the return type on a line of its own, because
tests/test_overlap_abi.py takes every one-line `int wgt_overlap_...(` for one of wgt_overlap_triangles' four
forms; the declarations are compared here with all white space folded."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from sanitize_driver import HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_overlap_self", "wgt_overlap_self_async", "wgt_overlap_self_stats", "wgt_overlap_self_spec")
FIELDS = ["hit", "count", "prim"]


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert "int wgt_overlap_self(wgt_ctx *ctx, const uint32_t *indices, uint32_t k, const wgt_overlap_buffers *out);" in flat
    assert ("int wgt_overlap_self_async(wgt_ctx *ctx, const uint32_t *d_indices, uint32_t k, "
            "const wgt_overlap_buffers *d_out, void *stream);") in flat
    assert ("int wgt_overlap_self_stats(wgt_ctx *ctx, const uint32_t *d_indices, uint32_t k, "
            "const wgt_overlap_buffers *d_out, uint64_t counts[2]);") in flat
    assert ("int wgt_overlap_self_spec(const wgt_triangle *tris, uint32_t n_tris, uint32_t first_prim, "
            "const uint32_t *indices, uint32_t k, const wgt_overlap_buffers *out);") in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version
    assert "wgt_overlap_self (the same, neighbours by index excluded)" in open(HEADER).read()  # the table's row


def test_every_header_entry_is_exported_and_bound(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    text = " ".join(re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S).split())
    assert set(re.findall(r"\bint (wgt_overlap_self\w*)\(", text)) == set(FUNCTIONS)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name  # a prototype, not ctypes' default
    assert [len(getattr(L, n).argtypes) for n in FUNCTIONS] == [4, 5, 5, 6]
    assert L.wgt_version() == 2


def test_struct_layout_matches_the_header(tmp_path):
    """The query answers into wgt_overlap_buffers, unchanged."""
    from webgputracer_amd import _lib

    lines = ['printf("size %zu\\n", sizeof(wgt_overlap_buffers));', 'printf("maxk %u\\n", (unsigned)WGT_OVERLAP_MAX_K);']
    lines += [f'printf("{f} %zu\\n", offsetof(wgt_overlap_buffers, {f}));' for f in FIELDS]
    head = '#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n'
    src = tmp_path / "sizes.c"
    src.write_text(head + "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    # the four prototypes, as a C compiler reads them (compiled, not linked)
    protos = ["int (*a)(wgt_ctx *, const uint32_t *, uint32_t, const wgt_overlap_buffers *) = wgt_overlap_self;",
              "int (*b)(wgt_ctx *, const uint32_t *, uint32_t, const wgt_overlap_buffers *, void *) = wgt_overlap_self_async;",
              "int (*c)(wgt_ctx *, const uint32_t *, uint32_t, const wgt_overlap_buffers *, uint64_t *) = wgt_overlap_self_stats;",
              "int (*d)(const wgt_triangle *, uint32_t, uint32_t, const uint32_t *, uint32_t, const wgt_overlap_buffers *) = "
              "wgt_overlap_self_spec;", "(void)a; (void)b; (void)c; (void)d;"]
    psrc = tmp_path / "protos.c"
    psrc.write_text(head + "\n".join(protos) + "\nreturn 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(psrc), "-o",
                    str(tmp_path / "protos.o")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 24 == ctypes.sizeof(_lib.WgtOverlapBuffers)
    assert [int(got[f]) for f in FIELDS] == [0, 8, 16] == [getattr(_lib.WgtOverlapBuffers, f).offset for f in FIELDS]
    assert int(got["maxk"]) == _lib.WGT_OVERLAP_MAX_K == 32


def test_null_context_is_refused_first(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    for f, args in ((L.wgt_overlap_self, (None, None, 99, None)),
                    (L.wgt_overlap_self_async, (None, None, 99, None, None)),
                    (L.wgt_overlap_self_stats, (None, None, 99, None, None))):
        assert f(*args) == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


def test_the_spec_refuses_in_order(wgt):
    """wgt_overlap_self_spec needs no device and runs check_overlap_self_args as the device forms do: no
    triangles succeeds before anything is looked at, then null triangles, then every refusal of the check in the
    header's order, each with its message; the first fault in that order is the one reported.  A null index
    buffer is no fault."""
    from webgputracer_amd import _lib

    L = _lib.lib()
    T = wgt.make_triangles(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.25, 0.25, -1], [0.25, 0.25, 1], [2, 2, 1]]], np.float32))
    idx = np.arange(6, dtype=np.uint32)
    word = np.zeros(80, np.uint32)
    tp, ip, wp = T.ctypes.data, idx.ctypes.data, word.ctypes.data
    B = _lib.WgtOverlapBuffers
    spec = L.wgt_overlap_self_spec
    assert spec(None, 0, 0, None, 99, None) == 0  # no triangles
    for args, text in (((None, 2, 0, ip, 1, ctypes.byref(B(prim=wp))), b"null triangles"),
                       ((tp, 2, 0, ip, 99, None), b"null output buffers"),
                       ((tp, 2, 0, ip, 99, ctypes.byref(B())), b"no overlap field asked for"),
                       ((tp, 2, 0, ip, 33, ctypes.byref(B(prim=wp))), b"k out of range"),
                       ((tp, 2, 0, ip, 33, ctypes.byref(B(hit=wp))), b"k out of range"),
                       ((tp, 2, 0, ip, 0, ctypes.byref(B(prim=wp))), b"prim asked for with k == 0"),
                       ((tp, 2, 0, None, 0, ctypes.byref(B(hit=wp, count=wp + 8, prim=wp + 16))), b"prim asked for with k == 0"),
                       ((tp, 2, 0, ip, 1, ctypes.byref(B(hit=wp))), b"k > 0 without prim"),
                       ((tp, 2, 0, None, 32, ctypes.byref(B(count=wp))), b"k > 0 without prim")):
        assert spec(*args) == _lib.WGT_E_INVALID and text in L.wgt_last_error(None), (text, L.wgt_last_error(None))
    assert not word.any()  # a refusal writes nothing
    for indices in (ip, None):
        word[:] = 0
        assert spec(tp, 2, 4, indices, 32, ctypes.byref(B(hit=wp, count=wp + 8, prim=wp + 16))) == 0
        assert list(word.view(np.uint8)[:2]) == [1, 1] and list(word[2:4]) == [1, 1]
        assert list(word[4:6]) == [5, 4] and (word[6:68] == 0xffffffff).all() and not word[68:].any()
    # the two triangles on one label are neighbours: nothing is reported
    shared = np.array([0, 1, 2, 3, 4, 2], np.uint32)
    assert spec(tp, 2, 4, shared.ctypes.data, 0, ctypes.byref(B(hit=wp, count=wp + 8))) == 0
    assert not word[:4].any()


def test_python_face(wgt):
    for name in ("overlap_self", "overlap_self_async", "overlap_self_stats", "self_intersections"):
        assert callable(getattr(wgt.Context, name)), name
    assert callable(wgt.overlap_self_spec) and "overlap_self_spec" in wgt.__all__
    T = wgt.make_triangles(np.array([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0.25, 0.25, -1], [0.25, 0.25, 1], [2, 2, 1]]], np.float32))
    with pytest.raises(ValueError):
        wgt.overlap_self_spec(T, None, 1, want=("prim", "dist"))
    with pytest.raises(ValueError, match="3 per triangle"):
        wgt.overlap_self_spec(T, np.arange(5), 1)
    got = wgt.overlap_self_spec(T[:0], None, 4)  # no triangles: empty arrays of the right shapes
    assert [got[f].shape for f in FIELDS] == [(0,), (0,), (0, 4)]
    got = wgt.overlap_self_spec(T, [[0, 1, 2], [3, 4, 5]], 3, first_prim=2)
    assert [got[f].shape for f in FIELDS] == [(2,), (2,), (2, 3)]
    assert [got[f].dtype for f in FIELDS] == [np.dtype(bool), np.dtype(np.uint32), np.dtype(np.uint32)]
    assert list(got["hit"]) == [True, True] and list(got["count"]) == [1, 1]
    assert list(got["prim"][0]) == [3, 0xffffffff, 0xffffffff] and list(got["prim"][1]) == [2, 0xffffffff, 0xffffffff]
    assert list(wgt.overlap_self_spec(T, want=("count",))["count"]) == [1, 1]  # the defaults: no indices, k = 0
    with pytest.raises(wgt.tracer.WgtError, match="k > 0 without prim"):
        wgt.overlap_self_spec(T, None, 3, want=("hit",))


PLAN_PROGRAM = r"""
#include <cstdio>
#include <string>
#include "webgputracer_amd/csrc/host/launch_plan.h"
using namespace wgt;
int main() {
  uint8_t b = 0;
  uint32_t w = 0;
  const wgt_overlap_buffers all{&b, &w, &w}, hit{&b, nullptr, nullptr}, none{nullptr, nullptr, nullptr};
  // every refusal of check_overlap_self_args, in the header's order: each line's fault and all later ones
  std::printf("check|%s\n", check_overlap_self_args(nullptr, 99));
  std::printf("check|%s\n", check_overlap_self_args(&none, 99));
  std::printf("check|%s\n", check_overlap_self_args(&all, 33));
  std::printf("check|%s\n", check_overlap_self_args(&all, 0));
  std::printf("check|%s\n", check_overlap_self_args(&hit, 1));
  std::printf("check|%s\n", check_overlap_self_args(&all, 32) ? "refused" : "fine");
  std::printf("check|%s\n", check_overlap_self_args(&hit, 0) ? "refused" : "fine");
  for (uint32_t stack : {1u, 7u, 32u, 225u, 256u})
    for (uint32_t k : {0u, 1u, 32u}) {
      DevScene sc{};
      sc.stack = stack;
      sc.n_tris = 200;
      OverlapSelfPlan p;
      const std::string bad = plan_overlap_self(sc, k ? &all : &hit, k, p);
      std::printf("plan|%u|%u|%u|%u|%u|%u|%s\n", stack, k, p.n, p.k, p.any, p.lds, bad.c_str());
    }
  return 0;
}
"""


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_plan(tmp_path):
    """check_overlap_self_args refuses in the header's order; plan_overlap_self gives one lane per resident
    triangle, the form, and 4 * 64 * (stack + k) bytes of LDS, and refuses a launch whose LDS exceeds one
    workgroup's 64 KiB (a stack no builder makes)."""
    src = tmp_path / "plan.cpp"
    src.write_text(PLAN_PROGRAM)
    exe = tmp_path / "plan"
    host = os.path.join(ROOT, "webgputracer_amd", "csrc", "host")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    "-I", ROOT, str(src), os.path.join(host, "bvh.cpp"), os.path.join(host, "launch_plan.cpp"), "-o", str(exe)],
                   check=True, timeout=600)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    checks = [ln.split("|", 1)[1] for ln in out if ln.startswith("check|")]
    assert checks == ["null output buffers", "no overlap field asked for", "k out of range (0..32)",
                      "prim asked for with k == 0", "k > 0 without prim", "fine", "fine"]
    plans = [ln.split("|")[1:] for ln in out if ln.startswith("plan|")]
    assert len(plans) == 15
    for stack, k, n, pk, any_, lds, bad in plans:
        stack, k = int(stack), int(k)
        assert int(n) == 200
        need = 4 * 64 * (stack + k)
        if need > 65536:
            assert "bytes of LDS" in bad and str(need) in bad and int(lds) == 0, (stack, k, bad)
        else:
            assert bad == "" and int(lds) == need and int(pk) == k and int(any_) == (1 if k == 0 else 0), (stack, k, bad)
    assert sum(1 for p in plans if p[6]) == 3  # 225 + 32, 256 + 1 and 256 + 32; 256 + 0 is 64 KiB exactly
