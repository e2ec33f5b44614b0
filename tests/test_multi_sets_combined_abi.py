"""CPU tier: the combined multi-signature check is exported with the signatures of include/bgls_hip.h, its argument checks need no
device, and without a usable GPU it refuses with BGLS_ERR_NO_DEVICE -- there is no silent fallback."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_verify_multi_sets_combined", "bgls_verify_multi_sets_combined_dev", "bgls_rlc_coefficients")


def test_combined_symbols_are_exported():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2
    header = open(os.path.join(ROOT, "include", "bgls_hip.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header, name


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    U64 = ctypes.c_uint64
    v = (ctypes.c_uint8 * 4)()
    seed = (ctypes.c_uint8 * 32)()
    zero = (U64 * 1)(0)
    one = (U64 * 2)(0, 1)
    two = (U64 * 3)(0, 1, 2)
    host = lambda n_sets, koff, moff, goff, n_groups, sd: lib.bgls_verify_multi_sets_combined(0, None, None, koff, n_sets, None, moff, goff, n_groups, sd, v, None)
    dev = lambda n_sets, goff, n_groups, sd: lib.bgls_verify_multi_sets_combined_dev(1, None, None, None, n_sets, 1, None, 32, 32, goff, n_groups, sd, v, None, None)
    # nothing to do
    assert host(0, zero, zero, None, 1, seed) == 0
    assert host(0, zero, zero, zero, 0, seed) == 0
    assert dev(0, None, 1, seed) == 0
    # non-monotone group_off
    assert host(2, two, two, (U64 * 4)(0, 2, 1, 2), 3, seed) == ERR_ARG
    assert dev(2, (U64 * 4)(0, 2, 1, 2), 3, seed) == ERR_ARG
    # group_off not ending at n_sets, not starting at 0
    assert host(2, two, two, (U64 * 3)(0, 1, 1), 2, seed) == ERR_ARG
    assert host(2, two, two, (U64 * 3)(0, 1, 3), 2, seed) == ERR_ARG
    assert host(2, two, two, (U64 * 3)(1, 1, 2), 2, seed) == ERR_ARG
    assert dev(2, (U64 * 3)(0, 1, 1), 2, seed) == ERR_ARG
    # NULL seed
    assert host(2, two, two, (U64 * 3)(0, 1, 2), 2, None) == ERR_ARG
    assert dev(2, None, 1, None) == ERR_ARG
    # NULL group_off with n_groups != 1
    assert host(2, two, two, None, 2, seed) == ERR_ARG
    assert host(2, two, two, None, 0, seed) == ERR_ARG
    assert dev(2, None, 2, seed) == ERR_ARG
    # the sibling call's own rules: key_off / msg_off monotone and non-NULL, 2^28 sets or more
    bad = (U64 * 3)(0, 2, 1)
    assert host(2, bad, two, None, 1, seed) == ERR_ARG
    assert host(2, two, bad, None, 1, seed) == ERR_ARG
    assert host(1, None, one, None, 1, seed) == ERR_ARG
    assert dev(1 << 28, None, 1, seed) == ERR_ARG
    # well-formed groups, NULL data: still an argument error, before any device work
    assert host(2, two, two, (U64 * 3)(0, 1, 2), 2, seed) == ERR_ARG
    assert dev(1, None, 1, seed) == ERR_ARG
    # the coefficients
    assert lib.bgls_rlc_coefficients(seed, 0, None) == 0
    assert lib.bgls_rlc_coefficients(None, 1, v) == ERR_ARG
    assert lib.bgls_rlc_coefficients(seed, 1, None) == ERR_ARG
    assert lib.bgls_rlc_coefficients(seed, 1 << 28, v) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
sig = (ctypes.c_uint8 * 64)()
key = (ctypes.c_uint8 * 128)()
msg = (ctypes.c_uint8 * 32)()
seed = (ctypes.c_uint8 * 32)()
r = (ctypes.c_uint8 * 16)()
koff = (ctypes.c_uint64 * 2)(0, 1)
moff = (ctypes.c_uint64 * 2)(0, 32)
v = (ctypes.c_uint8 * 1)()
print(lib.bgls_verify_multi_sets_combined(0, sig, key, koff, 1, msg, moff, None, 1, seed, v, None),
      lib.bgls_verify_multi_sets_combined_dev(0, ctypes.addressof(sig), ctypes.addressof(key), ctypes.addressof(koff), 1, 1, ctypes.addressof(msg), 32, 32,
                                              koff, 1, seed, v, None, None),
      lib.bgls_rlc_coefficients(seed, 1, r))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 3, r.stdout
