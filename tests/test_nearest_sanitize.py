"""The closest-point query's host side (the definition's brute force wgt_nearest_points_spec evaluates, over
the shared arithmetic of wgt_nearest.h, and the planning functions of wgt_nearest_points: its argument
checks in their order, the staging layout) built with AddressSanitizer + UBSan into a stand-alone
program and run over seeded random, degenerate, NaN and huge inputs
(tests/host_sanitize/nearest_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python is
sanitized, and the kernel is covered by tests/test_gpu_nearest.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_nearest_host_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "nearest_fuzz")
