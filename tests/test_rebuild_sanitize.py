"""The rebuild's host side (the specification BuildMortonBvh with the shared key and split arithmetic of
wgt_morton.h, and the planning functions of wgt_rebuild_triangles: its argument checks in their order,
the node capacity, the tree's and the scratch's layouts) built with AddressSanitizer + UBSan into a
stand-alone program and run over seeded random and degenerate meshes
(tests/host_sanitize/rebuild_fuzz.cpp).  CPU only, a plain process: nothing loaded into Python is
sanitized, and the kernels are covered by tests/test_gpu_rebuild.py."""
import os

import pytest

from sanitize_driver import HIPCC, run_sanitized


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_rebuild_host_under_asan_ubsan(tmp_path):
    run_sanitized(tmp_path, "rebuild_fuzz")
