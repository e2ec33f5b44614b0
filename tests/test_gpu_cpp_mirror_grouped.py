"""GPU tier: the C++ host mirror of the aggregate verification that pairs once per distinct message (include/bgls/bgls.hpp: GroupMessages,
VerifyAggregateSignatureGrouped, KoskVerifyAggregateSignatureGrouped) against the older mirror functions on the same inputs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_grouped.cpp")


@pytest.mark.gpu
def test_cpp_mirror_grouped(gpu_lib, tmp_path):
    exe = str(tmp_path / "test_grouped")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-L", os.path.join(ROOT, "bgls_amd"), "-lbgls_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "bgls_amd"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr
