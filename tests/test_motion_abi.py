"""The motion passes' C-ABI without a GPU: the header's declarations, the exports, the struct layout
and the refusals that need no device."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
FUNCTIONS = ("wgt_motion_snapshot", "wgt_motion_snapshot_read", "wgt_motion_reproject", "wgt_motion_reproject_async",
             "wgt_temporal_accumulate_motion", "wgt_temporal_accumulate_motion_async")


def test_header_declares_the_motion_passes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(rf"\b{name}\s*\(", text), name
    assert re.search(r"\}\s*wgt_motion_buffers\s*;", text)
    assert re.search(r"#define\s+WGT_API_VERSION\s+2\b", text)


def test_library_exports_the_motion_passes(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    exported = set(re.findall(r"\bT (wgt_\w+)", out.stdout))
    for name in FUNCTIONS:
        assert name in exported and name in _lib.EXPORTS and hasattr(L, name), name
    assert L.wgt_version() == 2


def test_struct_layout_matches_the_header(tmp_path):
    from webgputracer_amd import _lib

    fields = ["pos_prev", "norm_prev"]
    lines = ['printf("wgt_motion_buffers %zu\\n", sizeof(wgt_motion_buffers));', 'printf("hits %zu\\n", sizeof(wgt_hit_buffers));']
    lines += [f'printf("{f} %zu\\n", offsetof(wgt_motion_buffers, {f}));' for f in fields]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wgt_api.h"\nint main(void) {\n' +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert [f for f, _ in _lib.WgtMotionBuffers._fields_] == fields
    assert int(got["wgt_motion_buffers"]) == 16 == ctypes.sizeof(_lib.WgtMotionBuffers)
    assert [int(got[f]) for f in fields] == [0, 8] == [getattr(_lib.WgtMotionBuffers, f).offset for f in fields]
    assert int(got["hits"]) == 48 == ctypes.sizeof(_lib.WgtHitBuffers)  # unchanged


def test_null_context_is_refused(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    calls = ((L.wgt_motion_snapshot, (None, None)), (L.wgt_motion_snapshot_read, (None, None, 0)),
             (L.wgt_motion_reproject, (None, 1, None, None)), (L.wgt_motion_reproject_async, (None, 1, None, None, None)),
             (L.wgt_temporal_accumulate_motion, (None, None, 4, 4) + (None,) * 9),
             (L.wgt_temporal_accumulate_motion_async, (None, None, 4, 4) + (None,) * 10))
    for f, args in calls:
        assert f(*args) == _lib.WGT_E_INVALID
        assert b"null context" in L.wgt_last_error(None)


def test_python_face(wgt):
    for name in ("motion_snapshot", "motion_snapshot_read", "motion_reproject", "motion_reproject_async",
                 "temporal_accumulate_motion", "temporal_accumulate_motion_async"):
        assert callable(getattr(wgt.Context, name)), name
