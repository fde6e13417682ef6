"""The sampled renders' and the sample-map planner's planning functions (the argument checks in their
order, the budget cap from a histogram, the table of the sides' constants) built with AddressSanitizer
+ UBSan into a stand-alone program and run over seeded random and boundary arguments
(tests/host_sanitize/sampled_plan_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python is
sanitized, and the kernels are covered by tests/test_gpu_sampled.py and tests/test_gpu_sample_plan.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sampled_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "sampled_plan_fuzz")
