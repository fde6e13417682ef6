"""The planner of the pixel queue's order across launches (launch_plan.h OrderPlanner: which launch
makes its own order, which makes the kept one, which reuses it, and which shared buffer may be
rewritten) built with AddressSanitizer + UBSan into a stand-alone program and run over seeded random
sequences of launches, scene changes, resets and completions (tests/host_sanitize/order_plan_fuzz.cpp).
CPU only, a plain process: nothing loaded into Python is sanitized, and the launches themselves are
covered by tests/test_gpu_order_reuse.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_order_plan_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "order_plan_fuzz")
