"""The motion passes' planning functions (the argument checks of wgt_motion_reproject and of
wgt_temporal_accumulate_motion in their order) built with AddressSanitizer + UBSan into a stand-alone
program and run over seeded random and boundary arguments
(tests/host_sanitize/motion_plan_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python is
sanitized, and the kernels are covered by tests/test_gpu_motion.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_motion_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "motion_plan_fuzz")
