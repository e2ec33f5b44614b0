"""CPU tier: the batched pairing and the batched final exponentiation (one GT element per item) are exported with the signatures of
include/bgls_hip.h, check their arguments before they need a device, refuse without a usable GPU with BGLS_ERR_NO_DEVICE (no host
fallback), and have their Python and C++ mirrors."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_final_exp_batch", "bgls_final_exp_batch_dev", "bgls_pair_batch", "bgls_pair_batch_dev")


def test_symbols_are_exported_and_bound():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    b = (ctypes.c_uint8 * 576)()
    a = ctypes.addressof(b)
    # n == 0: nothing is looked at, not even the curve id's arrays
    assert lib.bgls_final_exp_batch(0, None, 0, None, None) == 0
    assert lib.bgls_final_exp_batch_dev(1, None, 0, None, None, None) == 0
    assert lib.bgls_pair_batch(1, None, None, 0, None) == 0
    assert lib.bgls_pair_batch_dev(0, None, None, 0, None, None) == 0
    # NULL arrays with n > 0, both outputs NULL
    assert lib.bgls_final_exp_batch(0, None, 1, b, b) == ERR_ARG
    assert lib.bgls_final_exp_batch(1, b, 1, None, None) == ERR_ARG
    assert lib.bgls_final_exp_batch_dev(0, None, 1, a, a, None) == ERR_ARG
    assert lib.bgls_final_exp_batch_dev(1, a, 1, None, None, None) == ERR_ARG
    assert lib.bgls_pair_batch(0, None, b, 1, b) == ERR_ARG
    assert lib.bgls_pair_batch(0, b, None, 1, b) == ERR_ARG
    assert lib.bgls_pair_batch(1, b, b, 1, None) == ERR_ARG
    assert lib.bgls_pair_batch_dev(0, None, a, 1, a, None) == ERR_ARG
    assert lib.bgls_pair_batch_dev(1, a, None, 1, a, None) == ERR_ARG
    assert lib.bgls_pair_batch_dev(1, a, a, 1, None, None) == ERR_ARG
    # the size cap of bgls_bb_verify_batch
    assert lib.bgls_final_exp_batch(0, b, 1 << 30, b, b) == ERR_ARG
    assert lib.bgls_final_exp_batch_dev(0, a, 1 << 30, a, a, None) == ERR_ARG
    assert lib.bgls_pair_batch(0, b, b, 1 << 30, b) == ERR_ARG
    assert lib.bgls_pair_batch_dev(0, a, a, 1 << 30, a, None) == ERR_ARG
    assert "too large" in _lib.last_error()


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
b = (ctypes.c_uint8 * 576)()
a = ctypes.addressof(b)
keep = (ctypes.c_uint8 * 576)(*([0x5a] * 576))
print(lib.bgls_final_exp_batch(0, b, 1, keep, keep), lib.bgls_final_exp_batch_dev(1, a, 1, a, None, None),
      lib.bgls_pair_batch(1, b, b, 1, keep), lib.bgls_pair_batch_dev(0, a, a, 1, a, None), bytes(keep) == b"\x5a" * 576)
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 4 + ["True"], r.stdout


def test_python_mirror_checks_lengths_before_the_library():
    from bgls_amd import Altbn128, Bls12
    import pytest
    for curve in (Altbn128, Bls12):
        assert hasattr(curve, "PairBatch")
        assert curve.PairBatch([], []) == []
        with pytest.raises(ValueError):
            curve.PairBatch([curve.GetG1Infinity()], [])


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "pb.cpp"
    src.write_text('#include "bgls/curves.hpp"\n'
                   "std::vector<curves::PointT> f(const curves::CurveSystem* c, const std::vector<curves::Point>& a, const std::vector<curves::Point>& b) {\n"
                   "  return c->PairBatch(a, b);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_pair_batch.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
