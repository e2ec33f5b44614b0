"""GPU tier: the C++ host mirror of the grouped aggregate verification over a resident key set (include/bgls/bgls.hpp:
KeySet::VerifyAggregateSignatureGroupedBySubset, KoskVerifyAggregateSignatureGroupedBySubset) against the older mirror functions on the
gathered keys."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_grouped_keys.cpp")


@pytest.mark.gpu
def test_cpp_mirror_grouped_keys(gpu_lib, tmp_path):
    exe = str(tmp_path / "test_grouped_keys")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-L", os.path.join(ROOT, "bgls_amd"), "-lbgls_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "bgls_amd"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
