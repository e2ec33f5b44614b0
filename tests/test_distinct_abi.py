"""CPU tier: the distinct-message and key-possession calls (hash inputs built on the device) are exported with the signatures of
include/bgls_hip.h, their argument checks need no device, and without a usable GPU a well-formed call refuses with BGLS_ERR_NO_DEVICE --
there is no silent fallback."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_hash_to_g1_keyed", "bgls_verify_aggregate_distinct", "bgls_verify_aggregate_distinct_h", "bgls_verify_aggregate_distinct_batch",
         "bgls_verify_aggregate_distinct_batch_dev", "bgls_verify_single_distinct_batch", "bgls_verify_single_distinct_batch_dev",
         "bgls_check_authentication_batch")


def test_distinct_symbols_are_exported():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2
    with open(os.path.join(ROOT, "include", "bgls_hip.h")) as f:
        header = f.read()
    for name in NAMES:
        assert "int %s(" % name in header, name


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    v = (ctypes.c_uint8 * 4)()
    g1 = (ctypes.c_uint8 * 192)()
    key = (ctypes.c_uint8 * 384)()
    msg = (ctypes.c_uint8 * 64)()
    zero = (ctypes.c_uint64 * 1)(0)
    bad = (ctypes.c_uint64 * 3)(0, 2, 1)
    good = (ctypes.c_uint64 * 3)(0, 1, 2)
    for cid in (0, 1):
        # the hash entry point: a mode outside 0 / 1, missing bytes and non-monotone offsets are refused (an empty batch goes on to the
        # device as bgls_hash_to_g1's does)
        assert lib.bgls_hash_to_g1_keyed(cid, 2, None, None, None, 0, None) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 2, key, msg, good, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, -1, key, msg, good, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 0, None, msg, good, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 0, key, msg, None, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 0, key, None, good, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 0, key, msg, good, 2, None) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 0, key, msg, bad, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 1, None, None, None, 2, g1) == ERR_ARG
        assert lib.bgls_hash_to_g1_keyed(cid, 0, key, msg, good, 1 << 30, g1) == ERR_ARG
        # the aggregate check from wire keys
        assert lib.bgls_verify_aggregate_distinct(cid, None, key, msg, good, 2) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct(cid, g1, None, msg, good, 2) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct(cid, g1, key, msg, None, 2) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct(cid, g1, key, None, good, 2) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct(cid, g1, key, msg, bad, 2) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct(cid, g1, key, msg, good, 1 << 30) == ERR_ARG
        # the batch of instances: bgls_verify_aggregate_batch's rules
        assert lib.bgls_verify_aggregate_distinct_batch(cid, None, None, zero, 0, None, zero, None, None) == 0
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, None, 2, msg, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, bad, 2, msg, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, good, 2, msg, bad, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, (ctypes.c_uint64 * 3)(1, 1, 2), 2, msg, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, None, key, good, 2, msg, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, None, good, 2, msg, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, good, 2, None, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, good, 2, msg, None, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, good, 2, msg, good, None, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch(cid, g1, key, (ctypes.c_uint64 * 2)(0, 1 << 30), 1, msg, good, v, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch_dev(cid, None, None, zero, 0, None, 0, 0, None, None, None) == 0
        assert lib.bgls_verify_aggregate_distinct_batch_dev(cid, None, None, None, 1, None, 32, 32, v, None, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch_dev(cid, None, None, bad, 2, None, 32, 32, v, None, None) == ERR_ARG
        assert lib.bgls_verify_aggregate_distinct_batch_dev(cid, None, None, good, 2, None, 32, 32, v, None, None) == ERR_ARG
        # the batch of single signatures: bgls_verify_multi_sets' rules
        assert lib.bgls_verify_single_distinct_batch(cid, None, None, None, zero, 0, None, None) == 0
        assert lib.bgls_verify_single_distinct_batch(cid, g1, key, msg, None, 2, v, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch(cid, g1, key, msg, bad, 2, v, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch(cid, None, key, msg, good, 2, v, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch(cid, g1, None, msg, good, 2, v, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch(cid, g1, key, None, good, 2, v, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch(cid, g1, key, msg, good, 2, None, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch(cid, g1, key, msg, good, 1 << 30, v, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch_dev(cid, None, None, 0, None, 0, 0, None, None, None) == 0
        assert lib.bgls_verify_single_distinct_batch_dev(cid, None, None, 2, None, 32, 32, v, None, None) == ERR_ARG
        assert lib.bgls_verify_single_distinct_batch_dev(cid, None, None, 1 << 30, None, 32, 32, v, None, None) == ERR_ARG
        # the authentication batch
        assert lib.bgls_check_authentication_batch(cid, None, None, 0, None, None) == 0
        assert lib.bgls_check_authentication_batch(cid, None, g1, 2, v, None) == ERR_ARG
        assert lib.bgls_check_authentication_batch(cid, key, None, 2, v, None) == ERR_ARG
        assert lib.bgls_check_authentication_batch(cid, key, g1, 2, None, None) == ERR_ARG
        assert lib.bgls_check_authentication_batch(cid, key, g1, 1 << 30, v, None) == ERR_ARG
    # an unknown key-set handle is an argument error, as for bgls_verify_aggregate_h
    assert lib.bgls_verify_aggregate_distinct_h(12345, g1, msg, good, 2, None) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
sig = (ctypes.c_uint8 * 64)()
key = (ctypes.c_uint8 * 128)()
msg = (ctypes.c_uint8 * 32)()
ioff = (ctypes.c_uint64 * 2)(0, 1)
moff = (ctypes.c_uint64 * 2)(0, 32)
v = (ctypes.c_uint8 * 1)()
a = ctypes.addressof
print(lib.bgls_hash_to_g1_keyed(0, 0, key, msg, moff, 1, sig),
      lib.bgls_hash_to_g1_keyed(0, 1, key, None, None, 1, sig),
      lib.bgls_verify_aggregate_distinct(0, sig, key, msg, moff, 1),
      lib.bgls_verify_aggregate_distinct_batch(0, sig, key, ioff, 1, msg, moff, v, None),
      lib.bgls_verify_aggregate_distinct_batch_dev(0, a(sig), a(key), ioff, 1, a(msg), 32, 32, v, None, None),
      lib.bgls_verify_single_distinct_batch(0, sig, key, msg, moff, 1, v, None),
      lib.bgls_verify_single_distinct_batch_dev(0, a(sig), a(key), 1, a(msg), 32, 32, v, None, None),
      lib.bgls_check_authentication_batch(0, key, sig, 1, v, None))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 8, r.stdout
