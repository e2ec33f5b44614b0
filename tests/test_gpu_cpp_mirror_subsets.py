"""GPU tier: the C++ host mirror of the multi-signature calls by signer subset (include/bgls/bgls.hpp: KeySet::AggregateKeysBySubset,
KeySet::VerifyMultiSignaturesBySubset, KeySet::KoskVerifyMultiSignaturesBySubset) against the single calls on the gathered keys."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_subsets.cpp")


@pytest.mark.gpu
def test_cpp_mirror_subsets(gpu_lib, tmp_path):
    exe = str(tmp_path / "test_subsets")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-L", os.path.join(ROOT, "bgls_amd"), "-lbgls_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "bgls_amd"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
