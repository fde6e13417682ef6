"""The sampled renders' and the sample-map planner's C-ABI without a GPU: the header's declarations and
its documented order of checks, the exports, the struct layout, the defaults, the workspace size and
the refusals that need no device (without one no context exists, so those are the NULL context's; the
rest of each call's order is run through the planning layer by tests/test_sampled_sanitize.py and
through the library by the GPU tests)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_render_tile_sampled", "wgt_render_tiles_sampled_async", "wgt_render_gbuffer_sampled",
             "wgt_render_gbuffer_sampled_async", "wgt_sample_plan_defaults", "wgt_sample_plan_workspace_bytes",
             "wgt_sample_plan", "wgt_sample_plan_async")
FIELDS = ["side_min", "side_max", "gain", "lum_floor", "min_history", "dilate", "budget_spp"]
DEFAULTS = [1, 8, 12.0, 1.0, 4, 2, 0.0]


def test_header_declares_the_calls():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
    assert re.search(r"\}\s*wgt_sample_plan_params\s*;", text)
    assert re.search(r"#define\s+WGT_API_VERSION\s+2\b", text)
    for name in ("wgt_render_tile", "wgt_render_tiles_async", "wgt_render_gbuffer", "wgt_render_gbuffer_async"):
        assert re.search(rf"\b{name}\s*\(", text), name  # the plain calls are declared as before


def test_header_lists_the_checks_in_order():
    text = open(HEADER).read()
    doc = text[text.index("wgt_sample_plan_workspace_bytes(uint32_t W"):text.index("int wgt_sample_plan(")]
    doc = " ".join(doc.replace("*", " ").split())
    order = ["NULL context", "NULL state", "NULL state->len or state->moments", "NULL map_out", "W or H 0 or above 32768",
             "parameters out of range", "(async) NULL workspace"]
    at = [doc.index(s) for s in order]
    assert at == sorted(at)
    doc = text[text.index("rendering with a per-pixel sample count"):text.index("int wgt_render_tile_sampled(")]
    doc = " ".join(doc.replace("*", " ").split())
    assert doc.index("everything the plain call checks") < doc.index("then a NULL map")


def test_library_exports_the_calls(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.wgt_version() == 2


def test_struct_sizes_match_the_header(tmp_path):
    from webgputracer_amd import _lib

    assert [f for f, _ in _lib.WgtSamplePlanParams._fields_] == FIELDS
    lines = ['printf("size %zu\\n", sizeof(wgt_sample_plan_params));', 'printf("stats %zu\\n", sizeof(wgt_stats));',
             'printf("state %zu\\n", sizeof(wgt_temporal_state));', 'printf("camera %zu\\n", sizeof(wgt_camera_param));']
    lines += [f'printf("{f} %zu\\n", offsetof(wgt_sample_plan_params, {f}));' for f in FIELDS]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == 28 == ctypes.sizeof(_lib.WgtSamplePlanParams)
    assert int(got["stats"]) == 232 == ctypes.sizeof(_lib.WgtStats)  # wgt_stats keeps its size
    assert int(got["state"]) == 24 and int(got["camera"]) == 48
    assert [int(got[f]) for f in FIELDS] == [0, 4, 8, 12, 16, 20, 24]
    for f in FIELDS:
        assert getattr(_lib.WgtSamplePlanParams, f).offset == int(got[f])


def test_defaults(wgt):
    from webgputracer_amd import _lib

    p = _lib.WgtSamplePlanParams(9, 9, 9.0, 9.0, 9, 9, 9.0)
    assert _lib.lib().wgt_sample_plan_defaults(ctypes.byref(p)) == 0
    assert [getattr(p, f) for f in FIELDS] == [ctypes.c_float(d).value if isinstance(d, float) else d for d in DEFAULTS]
    assert _lib.lib().wgt_sample_plan_defaults(None) == _lib.WGT_E_INVALID
    q = wgt.sample_plan_defaults()
    assert [getattr(q, f) for f in FIELDS] == [getattr(p, f) for f in FIELDS]


def test_workspace_bytes(wgt):
    sizes = [(1, 1), (1, 17), (5, 3), (64, 48), (67, 35), (130, 9), (1920, 1080), (32768, 1), (1, 32768), (32768, 1024),
             (8192, 4096)]
    sizes.sort(key=lambda s: s[0] * s[1])
    last = 0
    for w, h in sizes:
        b = wgt.sample_plan_workspace_bytes(w, h)
        assert b % 256 == 0 and b >= last and b >= w * h + 257 * 4, (w, h, b)
        last = b
    for w, h in ((0, 5), (5, 0), (32769, 1), (1, 32769), (8192, 8192), (32768, 1025)):
        assert wgt.sample_plan_workspace_bytes(w, h) == 0, (w, h)


def test_null_context_is_refused_first(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    calls = [lambda: L.wgt_render_tile_sampled(None, None, 0, 0, 0, 0, 0, 0, None, None, None, None, None),
             lambda: L.wgt_render_tiles_sampled_async(None, None, 0, 0, 0, 0, None, 1, None, None, None, None, None),
             lambda: L.wgt_render_gbuffer_sampled(None, None, 0, 0, 0, 0, 0, 0, None, None, None),
             lambda: L.wgt_render_gbuffer_sampled_async(None, None, 0, 0, 0, 0, None, 1, None, None, None, None),
             lambda: L.wgt_sample_plan(None, None, 0, 0, None, None, None),
             lambda: L.wgt_sample_plan_async(None, None, 0, 0, None, None, 0, None, None, None)]
    for call in calls:
        assert call() == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


def test_python_face(wgt):
    import inspect

    assert callable(wgt.sample_plan_defaults) and callable(wgt.sample_plan_workspace_bytes)
    assert callable(wgt.Context.sample_plan) and callable(wgt.Context.sample_plan_async)
    assert inspect.signature(wgt.Context.render_tile).parameters["sample_map"].default is None
    assert inspect.signature(wgt.Context.render_gbuffer).parameters["sample_map"].default is None
    assert inspect.signature(wgt.Context.render_tiles_async).parameters["d_sample_map"].default == 0
    assert inspect.signature(wgt.Context.render_gbuffer_async).parameters["d_sample_map"].default == 0
