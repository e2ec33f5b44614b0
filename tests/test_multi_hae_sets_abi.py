"""CPU tier: the batched HAE multi-signature verification and the per-set exponents are exported with the signatures of
include/bgls_hip.h; argument errors are found before any device work, and without a usable GPU the calls refuse with BGLS_ERR_NO_DEVICE --
there is no silent fallback."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_verify_multi_hae_sets", "bgls_verify_multi_hae_sets_dev", "bgls_hae_exponents_sets", "bgls_set_hae_root_host_min")


def test_multi_hae_sets_symbols_are_exported():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2
    assert lib.bgls_set_hae_root_host_min(2048) == 0


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    v = (ctypes.c_uint8 * 2)()
    t = (ctypes.c_uint8 * 64)()
    zero = (ctypes.c_uint64 * 1)(0)
    assert lib.bgls_verify_multi_hae_sets(0, None, None, zero, 0, None, zero, None, None, None) == 0
    assert lib.bgls_verify_multi_hae_sets_dev(1, None, None, None, 0, 0, None, 0, 0, None, None, None, None) == 0
    assert lib.bgls_hae_exponents_sets(0, None, zero, 0, None) == 0
    bad = (ctypes.c_uint64 * 3)(0, 2, 1)
    good = (ctypes.c_uint64 * 3)(0, 1, 2)
    assert lib.bgls_verify_multi_hae_sets(0, None, None, bad, 2, None, good, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_hae_sets(1, None, None, good, 2, None, bad, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_hae_sets(0, None, None, None, 1, None, zero, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_hae_sets(0, None, None, good, 2, None, good, v, None, None) == ERR_ARG     # keys NULL
    assert lib.bgls_verify_multi_hae_sets_dev(0, None, None, None, 1, 1, None, 32, 32, v, None, None, None) == ERR_ARG
    assert lib.bgls_hae_exponents_sets(0, None, bad, 2, t) == ERR_ARG
    assert lib.bgls_hae_exponents_sets(1, None, good, 2, t) == ERR_ARG                                     # keys NULL
    assert lib.bgls_hae_exponents_sets(1, None, None, 1, t) == ERR_ARG
    # a set of 2^28 keys (the XOF length 16 n is a uint32) and 2^30 keys in all are refused before anything is read
    big = (ctypes.c_uint64 * 2)(0, 1 << 28)
    assert lib.bgls_hae_exponents_sets(0, t, big, 1, t) == ERR_ARG
    assert lib.bgls_verify_multi_hae_sets(0, t, t, big, 1, t, (ctypes.c_uint64 * 2)(0, 1), v, None, None) == ERR_ARG
    many = (ctypes.c_uint64 * 6)(*[i * ((1 << 28) - 1) for i in range(6)])
    assert lib.bgls_hae_exponents_sets(0, t, many, 5, t) == ERR_ARG


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
t = (ctypes.c_uint8 * 16)()
print(lib.bgls_verify_multi_hae_sets(0, sig, key, koff, 1, msg, moff, v, None, None),
      lib.bgls_verify_multi_hae_sets_dev(0, ctypes.addressof(sig), ctypes.addressof(key), ctypes.addressof(koff), 1, 1, ctypes.addressof(msg), 32, 32,
                                         v, None, None, None),
      lib.bgls_hae_exponents_sets(0, key, koff, 1, t))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 3, r.stdout


def test_python_mirror_exists_and_takes_an_empty_batch():
    import pytest
    import bgls_amd
    from bgls_amd import bgls
    assert bgls.VerifyMultiSignaturesWithHAE(bgls_amd.Altbn128, [], [], []) == []
    with pytest.raises(ValueError):
        bgls.VerifyMultiSignaturesWithHAE(bgls_amd.Altbn128, [None], [], [])
