"""The self-intersection query's host side (plan_overlap_self: the argument checks in their order, one lane per
resident triangle, the form, the list length and the LDS bytes with its refusal; the staging layout of the
synchronous form; and the brute force wgt_overlap_self_spec on random, degenerate, NaN and out-of-range meshes
with and without labels and with every subset of the fields) built with AddressSanitizer + UBSan into a
stand-alone program and run as a plain child process (tests/host_sanitize/overlap_self_plan_fuzz.cpp).  CPU
only: nothing loaded into Python is sanitized, and the kernel is covered by tests/test_gpu_overlap_self.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_overlap_self_plan_and_spec_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "overlap_self_plan_fuzz")
