"""The queue order's C-ABI surface (include/wgt_api.h: wgt_order_info, wgt_order_read, wgt_order_reset):
declared, exported, bound, and refusing null arguments.  No compute here (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wgt_api.h")
NAMES = ("wgt_order_info", "wgt_order_read", "wgt_order_reset")


def test_header_declares_the_order_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    flat = " ".join(text.split())
    assert "int wgt_order_info(const wgt_ctx *ctx, wgt_order_stats *out);" in flat
    assert "int wgt_order_read(wgt_ctx *ctx, uint32_t *perm_out, uint32_t cap, uint32_t *n_out);" in flat
    assert "int wgt_order_reset(wgt_ctx *ctx);" in flat
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
    assert len(L.wgt_order_info.argtypes) == 2 and len(L.wgt_order_read.argtypes) == 4
    assert len(L.wgt_order_reset.argtypes) == 1


def test_order_stats_matches_the_header(tmp_path):
    from webgputracer_amd import _lib

    lines = ['printf("size %zu\\n", sizeof(wgt_order_stats));']
    for f, _ in _lib.WgtOrderStats._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(wgt_order_stats, {f}));')
    src = tmp_path / "sizes.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"wgt_api.h\"\nint main(void) {\n" +
                   "\n".join(lines) + "\nreturn 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(_lib.WgtOrderStats) == 40
    for f, _ in _lib.WgtOrderStats._fields_:
        assert int(got[f]) == getattr(_lib.WgtOrderStats, f).offset, f


def test_null_arguments_are_invalid(wgt):
    from webgputracer_amd import _lib

    L = _lib.lib()
    st = _lib.WgtOrderStats()
    n = ctypes.c_uint32(7)
    assert L.wgt_order_info(None, ctypes.byref(st)) == _lib.WGT_E_INVALID
    assert b"null" in L.wgt_last_error(None)
    assert L.wgt_order_read(None, None, 0, ctypes.byref(n)) == _lib.WGT_E_INVALID
    assert b"null" in L.wgt_last_error(None)
    assert L.wgt_order_read(None, None, 0, None) == _lib.WGT_E_INVALID
    assert L.wgt_order_reset(None) == _lib.WGT_E_INVALID
    assert b"null context" in L.wgt_last_error(None)


def test_python_face_has_the_calls(wgt):
    assert callable(wgt.Context.order_info) and callable(wgt.Context.order_read) and callable(wgt.Context.order_reset)
