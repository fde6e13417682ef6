"""The multi-hit query's planning functions (the argument checks of wgt_trace_multi_hits in their order, the
staging layout of its synchronous form, the launch's mode, list length and LDS bytes with its refusal)
built with AddressSanitizer + UBSan into a stand-alone program and run over seeded random and boundary
arguments (tests/host_sanitize/multihit_plan_fuzz.cpp).  CPU only, a plain process: nothing loaded into
Python is sanitized, and the kernel is covered by tests/test_gpu_multihit.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_multihit_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "multihit_plan_fuzz")
