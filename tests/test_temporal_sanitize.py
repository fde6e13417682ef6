"""The temporal accumulation's planning functions (the argument checks in their order, the overlap
test, the cameras' projection constants) built with AddressSanitizer + UBSan into a stand-alone
program and run over seeded random and boundary arguments
(tests/host_sanitize/temporal_plan_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python
is sanitized, and the kernel is covered by tests/test_gpu_temporal.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_temporal_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "temporal_plan_fuzz")
