"""The variance-guided denoiser's planning functions (the argument checks, the workspace layout, each
pass's constants) built with AddressSanitizer + UBSan into a stand-alone program and run over seeded
random and boundary arguments (tests/host_sanitize/denoise_variance_plan_fuzz.cpp).  CPU only, a
plain process: nothing loaded into Python is sanitized, and the kernels are covered by
tests/test_gpu_denoise_variance.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_denoise_variance_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "denoise_variance_plan_fuzz")
