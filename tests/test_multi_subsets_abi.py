"""CPU tier: the multi-signature calls by signer bitmap are declared in include/bgls_hip.h, exported with those signatures, refuse what
the arguments alone decide with BGLS_ERR_ARG before any device work, return 0 for an empty batch without touching a pointer, and
without a usable GPU refuse with BGLS_ERR_NO_DEVICE -- there is no silent fallback.  The refusals that need a key set (stride below
ceil(n / 8), a stray bit, a two-shard set) are in tests/test_gpu_multi_subsets.py: a handle only comes from an upload to a device."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_aggregate_subsets_h", "bgls_verify_multi_subsets_h", "bgls_verify_multi_subsets_keys_dev", "bgls_set_subset_complement")


def test_subset_symbols_are_declared_exported_and_in_signatures():
    from bgls_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "bgls_hip.h"), encoding="utf-8").read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    # the argument counts of the header and of SIGNATURES agree
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_empty_batch_returns_zero_without_touching_a_pointer():
    from bgls_amd import _lib
    lib = _lib.load()
    assert lib.bgls_aggregate_subsets_h(0, None, 0, 0, None) == 0
    assert lib.bgls_verify_multi_subsets_h(0, None, None, 0, 0, None, None, None, None, None) == 0
    assert lib.bgls_verify_multi_subsets_keys_dev(12345, None, None, 3, 0, None, 0, 0, None, None, None, None) == 0


def test_argument_errors_come_before_any_device_work():
    from bgls_amd import _lib
    lib = _lib.load()
    a = (ctypes.c_uint8 * 64)()
    v = (ctypes.c_uint8 * 4)()
    good = (ctypes.c_uint64 * 3)(0, 1, 2)
    bad = (ctypes.c_uint64 * 3)(0, 2, 1)
    p = ctypes.addressof(a)
    # NULL arrays with n_sets > 0
    assert lib.bgls_aggregate_subsets_h(1, None, 4, 2, a) == ERR_ARG
    assert lib.bgls_aggregate_subsets_h(1, a, 4, 2, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_h(1, None, a, 4, 2, a, good, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_h(1, a, None, 4, 2, a, good, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_h(1, a, a, 4, 2, a, None, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_h(1, a, a, 4, 2, a, good, None, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_h(1, a, a, 4, 2, None, good, v, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_h(1, a, a, 4, 2, a, bad, v, None, None) == ERR_ARG          # message offsets not monotone
    assert lib.bgls_verify_multi_subsets_keys_dev(1, None, p, 4, 2, p, 8, 8, v, None, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_keys_dev(1, p, None, 4, 2, p, 8, 8, v, None, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_keys_dev(1, p, p, 4, 2, None, 8, 8, v, None, None, None) == ERR_ARG
    assert lib.bgls_verify_multi_subsets_keys_dev(1, p, p, 4, 2, p, 8, 8, None, None, None, None) == ERR_ARG
    # the device form reads rows as 32-bit words: stride and pointer are multiples of 4
    assert p % 4 == 0
    for stride in (1, 2, 3, 5, 6, 7):
        assert lib.bgls_verify_multi_subsets_keys_dev(1, p, p, stride, 2, p, 8, 8, v, None, None, None) == ERR_ARG, stride
    for skew in (1, 2, 3):
        assert lib.bgls_verify_multi_subsets_keys_dev(1, p, p + skew, 4, 2, p, 8, 8, v, None, None, None) == ERR_ARG, skew
    # a batch of 2^30 sets or more
    assert lib.bgls_aggregate_subsets_h(1, a, 4, 1 << 30, a) == ERR_ARG
    # the mode switch
    assert lib.bgls_set_subset_complement(3) == ERR_ARG and lib.bgls_set_subset_complement(-1) == ERR_ARG
    for mode in (2, 1, 0):
        assert lib.bgls_set_subset_complement(mode) == 0


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
a = (ctypes.c_uint8 * 256)()
off = (ctypes.c_uint64 * 2)(0, 32)
v = (ctypes.c_uint8 * 1)()
p = ctypes.addressof(a)
print(lib.bgls_aggregate_subsets_h(1, a, 4, 1, a),
      lib.bgls_verify_multi_subsets_h(1, a, a, 4, 1, a, off, v, None, None),
      lib.bgls_verify_multi_subsets_keys_dev(1, p, p, 4, 1, p, 32, 32, v, None, None, None),
      lib.bgls_aggregate_subsets_h(1, None, 4, 1, a),
      lib.bgls_verify_multi_subsets_keys_dev(1, p, p, 6, 1, p, 32, 32, v, None, None, None),
      lib.bgls_aggregate_subsets_h(1, None, 0, 0, None))
"""


def test_no_device_means_an_error_not_a_fallback():
    """with the devices hidden: the no-device code for calls whose arguments are in order, the argument code where they are not, 0 for an empty batch"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 3 + [str(ERR_ARG)] * 2 + ["0"], r.stdout
