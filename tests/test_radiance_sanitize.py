"""The radiance query's planning functions (the argument checks of wgt_trace_radiance in their order, the
staging layout of its synchronous form, the launch's arguments and form) built with AddressSanitizer +
UBSan into a stand-alone program and run over seeded random and boundary arguments
(tests/host_sanitize/radiance_plan_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python is
sanitized, and the kernels are covered by tests/test_gpu_radiance.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_radiance_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "radiance_plan_fuzz")
