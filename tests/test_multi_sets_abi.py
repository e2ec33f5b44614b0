"""CPU tier: the batched multi-signature verification is exported with the signatures of include/bgls_hip.h, and without a usable GPU
it refuses with BGLS_ERR_NO_DEVICE -- there is no silent fallback.  The argument checks that need no device come first."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4


def test_multi_sets_symbols_are_exported():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in ("bgls_verify_multi_sets", "bgls_verify_multi_sets_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    v = (ctypes.c_uint8 * 2)()
    zero = (ctypes.c_uint64 * 1)(0)
    assert lib.bgls_verify_multi_sets(0, None, None, zero, 0, None, zero, None, None) == 0
    assert lib.bgls_verify_multi_sets_dev(1, None, None, None, 0, 0, None, 0, 0, None, None, None) == 0
    bad = (ctypes.c_uint64 * 3)(0, 2, 1)
    good = (ctypes.c_uint64 * 3)(0, 1, 2)
    assert lib.bgls_verify_multi_sets(0, None, None, bad, 2, None, good, v, None) == ERR_ARG
    assert lib.bgls_verify_multi_sets(1, None, None, good, 2, None, bad, v, None) == ERR_ARG
    assert lib.bgls_verify_multi_sets(0, None, None, None, 1, None, zero, v, None) == ERR_ARG
    assert lib.bgls_verify_multi_sets_dev(0, None, None, None, 1, 1, None, 32, 32, v, None, None) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
sig = (ctypes.c_uint8 * 64)()
key = (ctypes.c_uint8 * 128)()
msg = (ctypes.c_uint8 * 32)()
koff = (ctypes.c_uint64 * 2)(0, 1)
moff = (ctypes.c_uint64 * 2)(0, 32)
v = (ctypes.c_uint8 * 1)()
print(lib.bgls_verify_multi_sets(0, sig, key, koff, 1, msg, moff, v, None),
      lib.bgls_verify_multi_sets_dev(0, ctypes.addressof(sig), ctypes.addressof(key), ctypes.addressof(koff), 1, 1, ctypes.addressof(msg), 32, 32, v, None, None))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2, r.stdout
