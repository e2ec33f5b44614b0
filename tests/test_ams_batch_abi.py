"""CPU tier: the batched accountable-subgroup multisignature verification is exported with the signatures of include/bgls_hip.h; argument
errors are found before any device work, and without a usable GPU the calls refuse with BGLS_ERR_NO_DEVICE -- there is no silent
fallback."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_ams_verify_batch", "bgls_ams_verify_batch_dev", "bgls_set_ams_sum_cut")


def test_ams_batch_symbols_are_exported():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2
    assert lib.bgls_set_ams_sum_cut(0) == ERR_ARG
    assert lib.bgls_set_ams_sum_cut(1 << 16) == 0


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    v = (ctypes.c_uint8 * 2)()
    t = (ctypes.c_uint8 * 512)()
    idx = (ctypes.c_uint32 * 4)(0, 1, 2, 3)
    assert lib.bgls_ams_verify_batch(0, None, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.bgls_ams_verify_batch_dev(1, None, None, None, None, None, 0, 0, None, 0, 0, None, None, None) == 0
    bad = (ctypes.c_uint64 * 3)(0, 2, 1)
    good = (ctypes.c_uint64 * 3)(0, 1, 2)
    zero = (ctypes.c_uint64 * 2)(0, 0)
    assert lib.bgls_ams_verify_batch(0, t, t, t, idx, bad, 2, t, good, v, None) == ERR_ARG              # signer_off not monotone
    assert lib.bgls_ams_verify_batch(1, t, t, t, idx, good, 2, t, bad, v, None) == ERR_ARG              # msg_off not monotone
    assert lib.bgls_ams_verify_batch(0, t, t, t, idx, None, 1, t, zero, v, None) == ERR_ARG             # signer_off NULL
    assert lib.bgls_ams_verify_batch(0, t, t, t, None, good, 2, t, good, v, None) == ERR_ARG            # signers NULL, lists not empty
    assert lib.bgls_ams_verify_batch(0, None, t, t, idx, good, 2, t, good, v, None) == ERR_ARG          # apks NULL
    assert lib.bgls_ams_verify_batch(0, t, t, t, idx, good, 2, None, good, v, None) == ERR_ARG          # messages NULL, not empty
    # the device form: a list above max_signers, offsets that do not start at 0
    A = ctypes.addressof
    two = (ctypes.c_uint64 * 2)(0, 2)
    late = (ctypes.c_uint64 * 2)(1, 2)
    assert lib.bgls_ams_verify_batch_dev(0, A(t), A(t), A(t), A(idx), A(two), 1, 1, A(t), 8, 8, v, None, None) == ERR_ARG
    assert lib.bgls_ams_verify_batch_dev(1, A(t), A(t), A(t), A(idx), A(late), 1, 4, A(t), 8, 8, v, None, None) == ERR_ARG
    assert lib.bgls_ams_verify_batch_dev(0, A(t), A(t), A(t), A(idx), None, 1, 4, A(t), 8, 8, v, None, None) == ERR_ARG
    assert lib.bgls_ams_verify_batch_dev(0, A(t), A(t), A(t), None, A(two), 1, 2, A(t), 8, 8, v, None, None) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
sig = (ctypes.c_uint8 * 96)()
key = (ctypes.c_uint8 * 192)()
msg = (ctypes.c_uint8 * 32)()
idx = (ctypes.c_uint32 * 1)(7)
soff = (ctypes.c_uint64 * 2)(0, 1)
moff = (ctypes.c_uint64 * 2)(0, 32)
v = (ctypes.c_uint8 * 1)()
A = ctypes.addressof
print(lib.bgls_ams_verify_batch(0, key, key, sig, idx, soff, 1, msg, moff, v, None),
      lib.bgls_ams_verify_batch_dev(1, A(key), A(key), A(sig), A(idx), A(soff), 1, 1, A(msg), 32, 32, v, None, None))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2, r.stdout


def test_python_mirror_exists_and_takes_an_empty_batch():
    import pytest
    import bgls_amd
    from bgls_amd import bgls
    assert bgls.AmsVerifySignatures(bgls_amd.Altbn128, [], [], [], [], []) == []
    with pytest.raises(ValueError):
        bgls.AmsVerifySignatures(bgls_amd.Altbn128, [None], [], [], [], [])
    with pytest.raises(ValueError):
        bgls.AmsVerifySignatures(bgls_amd.Bls12, [], [], [], [], [b"m"])
