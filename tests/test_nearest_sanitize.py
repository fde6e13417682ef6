"""The closest-point query's host side (the definition's brute force wgt_nearest_points_spec evaluates, over
the shared arithmetic of wgt_nearest.h, and the planning functions of wgt_nearest_points: its argument
checks in their order, the staging layout) built with AddressSanitizer + UBSan into a stand-alone
program and run over seeded random, degenerate, NaN and huge inputs
(tests/host_sanitize/nearest_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python is
sanitized, and the kernel is covered by tests/test_gpu_nearest.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "webgputracer_amd", "csrc", "host")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_nearest_host_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "nearest_fuzz")
    srcs = [os.path.join(ROOT, "tests", "host_sanitize", "nearest_fuzz.cpp")] + [
        os.path.join(HOST, f) for f in ("bvh.cpp", "launch_plan.cpp")]
    # host-only compile: each sanitizer flag directly after -Xarch_host
    cmd = [HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
           "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"] + srcs + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "nearest_fuzz: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
