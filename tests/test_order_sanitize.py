"""The planner of the pixel queue's order across launches (launch_plan.h OrderPlanner: which launch
makes its own order, which makes the kept one, which reuses it, and which shared buffer may be
rewritten) built with AddressSanitizer + UBSan into a stand-alone program and run over seeded random
sequences of launches, scene changes, resets and completions (tests/host_sanitize/order_plan_fuzz.cpp).
CPU only, a plain process: nothing loaded into Python is sanitized, and the launches themselves are
covered by tests/test_gpu_order_reuse.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "webgputracer_amd", "csrc", "host")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_order_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "order_plan_fuzz")
    srcs = [os.path.join(ROOT, "tests", "host_sanitize", "order_plan_fuzz.cpp")] + [
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
    assert "order_plan_fuzz: ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
