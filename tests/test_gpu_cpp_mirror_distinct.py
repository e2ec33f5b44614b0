"""GPU tier: the C++ host mirror of the distinct-message and key-possession checks (include/bgls/bgls.hpp) against the older mirror
functions on messages prefixed by the test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_bgls_distinct.cpp")


@pytest.mark.gpu
def test_cpp_mirror_distinct(gpu_lib, tmp_path):
    exe = str(tmp_path / "test_bgls_distinct")
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), SRC, "-L", os.path.join(ROOT, "bgls_amd"), "-lbgls_hip",
                    "-Wl,-rpath," + os.path.join(ROOT, "bgls_amd"), "-o", exe], check=True, timeout=300)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout + out.stderr


def test_cpp_mirror_distinct_compiles():
    """CPU tier: the mirror's new functions compile against the C ABI (no GPU needed to build)."""
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), SRC], check=True, timeout=300)
