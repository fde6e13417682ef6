"""The one driver of the stand-alone sanitizer programs (tests/host_sanitize/*.cpp), for the
tests/test_*_sanitize.py: build one of them with the host sources it exercises under AddressSanitizer +
UBSan into an executable, run it as a plain child process, and assert that it built, exited 0, printed
its "<name>: ok" and that neither sanitizer reported.  CPU only; nothing loaded into Python is sanitized."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "webgputracer_amd", "csrc", "host")
HIPCC = "/opt/rocm/bin/hipcc"
PLAN_SOURCES = ("bvh.cpp", "launch_plan.cpp")  # what the planning layer's programs link


def run_sanitized(tmp_path, name, host_sources=PLAN_SOURCES, fp_contract_off=True, libs=()):
    """name: the program (tests/host_sanitize/<name>.cpp); host_sources: files of csrc/host built with it;
    fp_contract_off: the product's -ffp-contract=off; libs: linker flags after the output."""
    exe = str(tmp_path / name)
    srcs = [os.path.join(ROOT, "tests", "host_sanitize", name + ".cpp")] + [os.path.join(HOST, f) for f in host_sources]
    # host-only compile: each sanitizer flag directly after -Xarch_host
    cmd = ([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer"]
           + (["-ffp-contract=off"] if fp_contract_off else [])
           + ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
              "-fsanitize=undefined", "-Xarch_host", "-fno-sanitize-recover=all"] + srcs + ["-o", exe] + list(libs))
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert name + ": ok" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
