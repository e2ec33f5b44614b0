"""CPU tier: the grouped aggregate verification over a resident key set by signer bitmap is declared in include/bgls_hip.h, exported with
those signatures, refuses what the arguments alone decide with BGLS_ERR_ARG before any device work, and without a usable GPU refuses
with BGLS_ERR_NO_DEVICE -- there is no silent fallback.  The refusals that need a key set (a short bitmap, a stray bit, a popcount other
than n_msgs, a two-shard set) are in tests/test_gpu_verify_aggregate_grouped_keys.py: a handle only comes from an upload to a device."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_verify_aggregate_grouped_h", "bgls_verify_aggregate_grouped_keys_dev", "bgls_set_group_small")
SIZE_MAX = ctypes.c_size_t(-1).value


def test_symbols_are_declared_exported_and_in_signatures():
    from bgls_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "bgls_hip.h"), encoding="utf-8").read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        decl = re.search(r"^int %s\((.*?)\);" % name, header, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name][1]), name


def test_no_stage_is_appended_and_the_pure_pieces_have_their_header():
    core = open(os.path.join(ROOT, "bgls_amd", "csrc", "engine_core.inc"), encoding="utf-8").read()
    assert re.search(r'"rlc",\s*"group"\}', core), "the selection pass runs under the group stage: the list still ends there"
    assert os.path.exists(os.path.join(ROOT, "bgls_amd", "csrc", "grpkeys.hpp"))


def test_argument_errors_come_before_any_device_work():
    from bgls_amd import _lib
    lib = _lib.load()
    a = (ctypes.c_uint8 * 256)()
    good = (ctypes.c_uint64 * 3)(0, 1, 2)
    bad = (ctypes.c_uint64 * 3)(0, 2, 1)
    p = ctypes.addressof(a)
    assert p % 4 == 0
    d = ctypes.c_size_t(0)
    h = 1
    # host form: NULL sig, NULL offsets (also for n_msgs = 0), NULL blob with bytes to read, offsets not monotone, 2^30 messages
    assert lib.bgls_verify_aggregate_grouped_h(h, None, a, 4, a, good, 2, ctypes.byref(d), None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, a, 4, a, None, 2, ctypes.byref(d), None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, a, 4, a, None, 0, ctypes.byref(d), None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, None, 0, a, None, 0, None, None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, a, 4, None, good, 2, ctypes.byref(d), None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, a, 4, a, bad, 2, ctypes.byref(d), None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, a, 4, a, good, 1 << 30, ctypes.byref(d), None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_h(h, a, None, 0, a, good, 1 << 30, None, None) == ERR_ARG
    # device form: NULL d_sig, NULL d_msgs with messages, a stride below the length, 2^30 messages
    assert lib.bgls_verify_aggregate_grouped_keys_dev(h, None, p, 4, p, 8, 8, 2, ctypes.byref(d), None, None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_keys_dev(h, p, p, 4, None, 8, 8, 2, ctypes.byref(d), None, None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_keys_dev(h, p, None, 0, None, 8, 8, 2, None, None, None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_keys_dev(h, p, p, 4, p, 8, 7, 2, ctypes.byref(d), None, None) == ERR_ARG
    assert lib.bgls_verify_aggregate_grouped_keys_dev(h, p, p, 4, p, 8, 8, 1 << 30, ctypes.byref(d), None, None) == ERR_ARG
    # the device form reads the bitmap as 32-bit words: length and pointer are multiples of 4
    for length in (1, 2, 3, 5, 6, 7):
        assert lib.bgls_verify_aggregate_grouped_keys_dev(h, p, p, length, p, 8, 8, 2, None, None, None) == ERR_ARG, length
    for skew in (1, 2, 3):
        assert lib.bgls_verify_aggregate_grouped_keys_dev(h, p, p + skew, 4, p, 8, 8, 2, None, None, None) == ERR_ARG, skew


def test_the_threshold_switch_answers_with_or_without_a_device():
    from bgls_amd import _lib
    lib = _lib.load()
    try:
        for k in (0, 8, SIZE_MAX):
            assert lib.bgls_set_group_small(k) == 0, k
    finally:
        lib.bgls_set_group_small(32)


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
a = (ctypes.c_uint8 * 512)()
off = (ctypes.c_uint64 * 3)(0, 32, 64)
bad = (ctypes.c_uint64 * 3)(0, 64, 32)
d = ctypes.c_size_t(7)
p = ctypes.addressof(a)
print(lib.bgls_verify_aggregate_grouped_h(1, a, a, 4, a, off, 2, ctypes.byref(d), None),
      lib.bgls_verify_aggregate_grouped_h(1, a, None, 0, a, off, 2, ctypes.byref(d), None),
      lib.bgls_verify_aggregate_grouped_h(1, a, a, 4, a, off, 0, ctypes.byref(d), None),
      lib.bgls_verify_aggregate_grouped_keys_dev(1, p, p, 4, p, 32, 32, 2, ctypes.byref(d), None, None),
      lib.bgls_verify_aggregate_grouped_keys_dev(1, p, None, 0, p, 32, 32, 2, ctypes.byref(d), None, None),
      lib.bgls_verify_aggregate_grouped_h(1, a, a, 4, a, bad, 2, ctypes.byref(d), None),
      lib.bgls_verify_aggregate_grouped_h(1, None, a, 4, a, off, 2, ctypes.byref(d), None),
      lib.bgls_verify_aggregate_grouped_keys_dev(1, p, p, 6, p, 32, 32, 2, ctypes.byref(d), None, None),
      lib.bgls_verify_aggregate_grouped_keys_dev(1, p, p, 4, p, 32, 31, 2, ctypes.byref(d), None, None),
      lib.bgls_set_group_small(0), lib.bgls_set_group_small(32))
"""


def test_no_device_means_an_error_not_a_fallback():
    """with the devices hidden: the no-device code for calls whose arguments are in order (whatever the handle: it is not looked at), the
    argument code where they are not, 0 for the threshold switch"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 5 + [str(ERR_ARG)] * 4 + ["0", "0"], r.stdout
