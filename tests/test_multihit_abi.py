"""The multi-hit query's C-ABI surface (include/wgt_api.h: wgt_trace_multi_hits and its forms): declared,
exported, bound, the struct's layout against the header, the order of the argument checks as the planning
function (host/launch_plan.h check_multi_hit_args) applies it, and the refusal that needs no scene.  No
compute on a device (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_trace_multi_hits", "wgt_trace_multi_hits_async", "wgt_trace_multi_hits_stats")
FIELDS = ["count", "prim", "dist"]


def test_header_declares_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert ("int wgt_trace_multi_hits(wgt_ctx *ctx, const float *rays, const float *max_dist, uint32_t n, uint32_t k, "
            "uint32_t flags, const wgt_multi_hit_buffers *out);") in flat
    assert ("int wgt_trace_multi_hits_async(wgt_ctx *ctx, const float *d_rays, const float *d_max_dist, uint32_t n, "
            "uint32_t k, uint32_t flags, const wgt_multi_hit_buffers *d_out, void *stream);") in flat
    assert ("int wgt_trace_multi_hits_stats(wgt_ctx *ctx, const float *d_rays, const float *d_max_dist, uint32_t n, "
            "uint32_t k, uint32_t flags, const wgt_multi_hit_buffers *d_out, uint64_t counts[2]);") in flat
    assert "#define WGT_MULTI_HIT_TRIS_ONLY 1u" in flat and "#define WGT_MULTI_HIT_MAX_K 32u" in flat
    assert "#define WGT_API_VERSION 2" in text  # adding functions keeps the version
    assert "wgt_trace_multi_hits (the k nearest hits" in open(HEADER).read()  # the table's row


def test_library_exports_and_binding_names_them(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name  # a prototype, not ctypes' default
    assert [len(getattr(L, n).argtypes) for n in FUNCTIONS] == [7, 8, 8]
    assert L.wgt_version() == 2


def test_struct_layout_matches_the_header(tmp_path):
    from webgputracer_amd import _lib

    lines = ['printf("size %zu\\n", sizeof(wgt_multi_hit_buffers));', 'printf("hits %zu\\n", sizeof(wgt_hit_buffers));',
             'printf("nearest %zu\\n", sizeof(wgt_nearest_buffers));',
             'printf("radiance %zu\\n", sizeof(wgt_radiance_buffers));',
             'printf("flag %u\\n", WGT_MULTI_HIT_TRIS_ONLY);', 'printf("maxk %u\\n", WGT_MULTI_HIT_MAX_K);']
    lines += [f'printf("{f} %zu\\n", offsetof(wgt_multi_hit_buffers, {f}));' for f in FIELDS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in _lib.WgtMultiHitBuffers._fields_] == FIELDS == list(_lib.MULTI_HIT_FIELDS)
    assert int(got["size"]) == 24 == ctypes.sizeof(_lib.WgtMultiHitBuffers)
    assert [int(got[f]) for f in FIELDS] == [0, 8, 16] == [getattr(_lib.WgtMultiHitBuffers, f).offset for f in FIELDS]
    assert int(got["hits"]) == 48 and int(got["nearest"]) == 32 and int(got["radiance"]) == 24  # unchanged
    assert int(got["flag"]) == _lib.WGT_MULTI_HIT_TRIS_ONLY == 1 and int(got["maxk"]) == _lib.WGT_MULTI_HIT_MAX_K == 32


def test_null_context_is_refused_first(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    for f, args in ((L.wgt_trace_multi_hits, (None, None, None, 1, 99, 0xff, None)),
                    (L.wgt_trace_multi_hits_async, (None, None, None, 1, 99, 0xff, None, None)),
                    (L.wgt_trace_multi_hits_stats, (None, None, None, 1, 99, 0xff, None, None))):
        assert f(*args) == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


PLAN_PROBE = r"""
#include <cstdint>
#include <cstdio>
#include "wgt_api.h"
namespace wgt { const char* check_multi_hit_args(const void* rays, const wgt_multi_hit_buffers* out, uint64_t k, uint64_t flags); }
int main() {
  float ray = 0.0f; uint32_t word = 0;
  const wgt_multi_hit_buffers none{}, count{&word, nullptr, nullptr}, prim{nullptr, &word, nullptr},
      dist{nullptr, nullptr, &ray};
  const struct { const void* rays; const wgt_multi_hit_buffers* out; uint64_t k, flags; } c[] = {
      {nullptr, nullptr, 99, 2}, {&ray, nullptr, 99, 2}, {&ray, &none, 99, 2}, {&ray, &prim, 99, 2}, {&ray, &prim, 99, 1},
      {&ray, &prim, 0, 0}, {&ray, &dist, 33, 0}, {&ray, &dist, 32, 1}, {&ray, &prim, 1, 0}, {&ray, &count, 99, 0},
      {&ray, &count, 0, 1}, {&ray, &count, 0, 2}};
  for (const auto& k : c) {
    const char* r = wgt::check_multi_hit_args(k.rays, k.out, k.k, k.flags);
    std::printf("%s\n", r ? r : "fine");
  }
  return 0;
}
"""


def test_the_order_of_the_argument_checks(wgt, tmp_path):
    """After the context, the scene and n == 0, which the entry points check themselves: null rays, a null
    struct, a struct without a field, unknown flag bits, then k, which only prim and dist need; each refusal
    names its argument.  The planning function is the library's own (the entry points pass its text to the
    caller), called from a small program."""
    from webgputracer_amd import _lib

    src = tmp_path / "probe.cpp"
    src.write_text(PLAN_PROBE)
    exe = tmp_path / "probe"
    libdir = os.path.dirname(os.path.abspath(_lib.LIB_PATH))
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L", libdir,
                    "-l:" + os.path.basename(_lib.LIB_PATH), "-Wl,-rpath," + libdir], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = ["null rays", "null output buffers", "no multi-hit field", "unknown multi-hit flags", "k out of range",
            "k out of range", "k out of range", "fine", "fine", "fine", "fine", "unknown multi-hit flags"]
    assert len(got) == len(want) and all(w in g for w, g in zip(want, got)), got


def test_python_face(wgt):
    import pytest

    for name in ("trace_multi_hits", "trace_multi_hits_async", "trace_multi_hits_stats", "points_inside"):
        assert callable(getattr(wgt.Context, name)), name
    from webgputracer_amd import frames

    assert callable(frames.render_hit_count)
    with pytest.raises(SystemExit):  # --hit-count excludes the other outputs, before any device is touched
        frames.main(["--hit-count", "--gbuffer", "--out", "x"])
    with pytest.raises(SystemExit):
        frames.main(["--hit-count", "--panorama", "--out", "x"])
    with pytest.raises(SystemExit):  # and needs somewhere to write
        frames.main(["--hit-count"])
