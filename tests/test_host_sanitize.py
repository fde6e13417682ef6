"""The product's host code (BVH builder, OBJ parser, procedural meshes, host C-ABI, and the
planning layer of the device calls: limits, frame constants, kernel form, scene layout) built
with AddressSanitizer + UBSan and run over random, degenerate and malformed inputs
(tests/host_sanitize/host_fuzz.cpp).  CPU only: GPU sanitizers are not available on the
GPU pool, and the device code is covered by the -m gpu parity suite instead."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_host_code_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "host_fuzz",
                  ("bvh.cpp", "obj_loader.cpp", "procedural.cpp", "host_api.cpp", "scene.cpp", "objects.cpp",
                   "launch_plan.cpp"), fp_contract_off=False, libs=("-lz",))
