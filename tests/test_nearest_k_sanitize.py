"""The k-nearest closest-point query's host side (the argument checks of wgt_nearest_k_points in their order,
the staging layout of its synchronous form, the launch's mode, list length and LDS bytes with its refusal,
and the brute force wgt_nearest_k_points_spec on random, degenerate, NaN and huge inputs with every subset
of the fields at k = 1 and 32) built with AddressSanitizer + UBSan into a stand-alone program and run as a
plain child process (tests/host_sanitize/nearest_k_fuzz.cpp).  CPU only: nothing loaded into Python is
sanitized, and the kernel is covered by tests/test_gpu_nearest_k.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_nearest_k_spec_and_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "nearest_k_fuzz")
