"""The host side of the BVH refit (RefitBvh and the update's planning functions) built with
AddressSanitizer + UBSan into a stand-alone program and run over seeded random meshes and motions,
non-finite input included (tests/host_sanitize/refit_fuzz.cpp).  CPU only, a plain process: nothing
loaded into Python is sanitized, and the device kernels are covered by tests/test_gpu_refit.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_refit_host_code_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "refit_fuzz")
