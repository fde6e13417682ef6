"""The temporal accumulation's C-ABI without a GPU: the header's declarations, the exports, the struct
layouts, the defaults and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_temporal_defaults", "wgt_temporal_accumulate", "wgt_temporal_accumulate_async")


def test_header_declares_the_accumulation():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
    assert re.search(r"#define\s+WGT_TEMPORAL_MATCH_PRIM\s+1u", text)
    assert re.search(r"\}\s*wgt_temporal_params\s*;", text) and re.search(r"\}\s*wgt_temporal_state\s*;", text)
    assert re.search(r"#define\s+WGT_API_VERSION\s+2\b", text)


def test_library_exports_the_accumulation(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.wgt_version() == 2


def test_struct_layouts_match_the_header(tmp_path):
    from webgputracer_amd import _lib

    structs = {"wgt_temporal_params": (_lib.WgtTemporalParams, ["max_history", "normal_min", "plane_tol", "flags"], 16,
                                       [0, 4, 8, 12]),
               "wgt_temporal_state": (_lib.WgtTemporalState, ["rgba32f", "len", "moments"], 24, [0, 8, 16])}
    lines = ['printf("flag %u\\n", WGT_TEMPORAL_MATCH_PRIM);']
    for name, (_, fields, _, _) in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["flag"]) == 1 == _lib.WGT_TEMPORAL_MATCH_PRIM
    for name, (cls, fields, size, offsets) in structs.items():
        assert [f for f, _ in cls._fields_] == fields
        assert int(got[name]) == size == ctypes.sizeof(cls), name
        assert [int(got[f"{name}.{f}"]) for f in fields] == offsets == [getattr(cls, f).offset for f in fields], name


def test_defaults(wgt):
    from webgputracer_amd import _lib

    p = _lib.WgtTemporalParams(9, 9.0, 9.0, 9)
    assert _lib.lib().wgt_temporal_defaults(ctypes.byref(p)) == 0
    assert (p.max_history, p.normal_min, p.plane_tol, p.flags) == (32, ctypes.c_float(0.9).value, 1.0, 0)
    assert _lib.lib().wgt_temporal_defaults(None) == _lib.WGT_E_INVALID
    q = wgt.temporal_defaults()
    assert (q.max_history, q.normal_min, q.plane_tol, q.flags) == (32, ctypes.c_float(0.9).value, 1.0, 0)


def test_null_context_is_refused(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    assert L.wgt_temporal_accumulate(None, None, 4, 4, None, None, None, None, None, None, None, None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)
    assert (L.wgt_temporal_accumulate_async(None, None, 4, 4, None, None, None, None, None, None, None, None, None) ==
            _lib.WGT_E_INVALID)
    assert b"null context" in L.wgt_last_error(None)


def test_python_face(wgt):
    import inspect

    assert callable(wgt.temporal_defaults)
    assert callable(wgt.Context.temporal_accumulate) and callable(wgt.Context.temporal_accumulate_async)
    # camera_param's new keywords default to the constants it always wrote
    sig = inspect.signature(wgt.camera_param)
    assert sig.parameters["origin"].default == (278.0, 278.0, -800.0)
    assert sig.parameters["target"].default == (278.0, 278.0, 0.0)
    cam = wgt.camera_param(1.5, 4, 7)
    assert cam["origin"].tolist() == [[278.0, 278.0, -800.0]] and cam["target"].tolist() == [[278.0, 278.0, 0.0]]
    moved = wgt.camera_param(1.5, 4, 7, origin=(1.0, 2.0, 3.0), target=(4.0, 5.0, 6.0))
    assert moved["origin"].tolist() == [[1.0, 2.0, 3.0]] and moved["target"].tolist() == [[4.0, 5.0, 6.0]]
    assert (moved["aspect"], moved["spp"], moved["seed"]) == (cam["aspect"], cam["spp"], cam["seed"])
