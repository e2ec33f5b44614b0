"""CPU tier: key sets from compressed keys -- bgls_decompress_points_dev, bgls_keys_upload_compressed and bgls_keys_read are exported with
the signatures of include/bgls_hip.h, check their arguments in the documented order before they need a device, leave first_bad alone
on every argument error, refuse without a usable GPU with BGLS_ERR_NO_DEVICE (no host fallback), and have their Python and C++ mirrors."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_decompress_points_dev", "bgls_keys_upload_compressed", "bgls_keys_read")
KEEP = 0x5A5A5A5A


def test_symbols_are_exported_and_bound():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    header = open(os.path.join(ROOT, "include", "bgls_hip.h")).read()
    for name in NAMES:
        assert "int %s(" % name in header


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    b = (ctypes.c_uint8 * 192)()
    a = ctypes.addressof(b)
    # n == 0: nothing is looked at, neither a pointer nor the group nor the curve id
    assert lib.bgls_decompress_points_dev(0, 2, None, 0, None, None, None) == 0
    assert lib.bgls_decompress_points_dev(7, 9, None, 0, None, None, None) == 0
    # the size cap comes first, then the group and the pointers, then the curve
    assert lib.bgls_decompress_points_dev(0, 2, None, 1 << 30, None, None, None) == ERR_ARG
    assert "too large" in _lib.last_error()
    assert lib.bgls_decompress_points_dev(0, 2, None, 1, a, a, None) == ERR_ARG
    assert lib.bgls_decompress_points_dev(0, 2, a, 1, None, a, None) == ERR_ARG
    assert lib.bgls_decompress_points_dev(1, 1, a, 1, a, None, None) == ERR_ARG
    assert lib.bgls_decompress_points_dev(0, 3, a, 1, a, a, None) == ERR_ARG
    assert "group" in _lib.last_error()

    h = ctypes.c_uint64(KEEP)
    bad = ctypes.c_size_t(KEEP)
    one = (ctypes.c_int * 1)(0)
    assert lib.bgls_keys_upload_compressed(0, b, 1 << 30, one, 1, 0, ctypes.byref(h), ctypes.byref(bad)) == ERR_ARG
    assert "too large" in _lib.last_error()
    assert lib.bgls_keys_upload_compressed(0, b, 1, one, 1, 0, None, ctypes.byref(bad)) == ERR_ARG
    assert lib.bgls_keys_upload_compressed(0, None, 1, one, 1, 0, ctypes.byref(h), ctypes.byref(bad)) == ERR_ARG
    assert lib.bgls_keys_upload_compressed(0, b, 1, one, 0, 0, ctypes.byref(h), ctypes.byref(bad)) == ERR_ARG
    assert lib.bgls_keys_upload_compressed(0, b, 1, one, 17, 0, ctypes.byref(h), ctypes.byref(bad)) == ERR_ARG
    assert "n_devices" in _lib.last_error()
    assert lib.bgls_keys_upload_compressed(5, b, 1, one, 1, 0, ctypes.byref(h), ctypes.byref(bad)) == ERR_ARG
    assert "curve" in _lib.last_error()
    assert h.value == KEEP and bad.value == KEEP

    assert lib.bgls_keys_read(0xDEAD, 0, 0, b) == ERR_ARG
    assert "handle" in _lib.last_error()
    assert lib.bgls_keys_read(0, 0, 1, None) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
b = (ctypes.c_uint8 * 192)()
a = ctypes.addressof(b)
h, bad = ctypes.c_uint64(77), ctypes.c_size_t(77)
print(lib.bgls_decompress_points_dev(0, 2, a, 1, a, a, None), lib.bgls_decompress_points_dev(1, 1, a, 1, a, a, None),
      lib.bgls_keys_upload_compressed(0, b, 1, None, 1, 0, ctypes.byref(h), ctypes.byref(bad)),
      lib.bgls_keys_upload_compressed(1, b, 0, None, 1, 2, ctypes.byref(h), ctypes.byref(bad)), h.value, bad.value)
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 4 + ["77", "77"], r.stdout


def test_python_mirror_is_there_and_checks_the_length_first():
    import pytest
    from bgls_amd import Altbn128, bgls
    assert callable(bgls.KeySet.from_compressed) and callable(bgls.KeySet.keys)
    with pytest.raises(ValueError, match="multiple of 64"):
        bgls.KeySet.from_compressed(Altbn128, bytes(65))


def test_cpp_mirror_compiles(tmp_path):
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_keys_compressed.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
