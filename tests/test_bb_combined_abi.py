"""CPU tier: the combined Boneh-Boyen check is exported with the signatures of include/bgls_hip.h, its argument checks need no device,
without a usable GPU it refuses with BGLS_ERR_NO_DEVICE -- there is no silent fallback -- and it has its Python and C++ mirrors."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4
NAMES = ("bgls_bb_verify_batch_combined", "bgls_bb_verify_batch_combined_dev")


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
    b = (ctypes.c_uint8 * 512)()
    seed = (ctypes.c_uint8 * 32)()
    p = ctypes.addressof(b)
    host = lambda n, goff, n_groups, sd, arr=b: lib.bgls_bb_verify_batch_combined(0, arr, arr, arr, arr, n, goff, n_groups, sd, v, None)
    dev = lambda n, goff, n_groups, sd, arr=p: lib.bgls_bb_verify_batch_combined_dev(1, arr, arr, arr, arr, n, goff, n_groups, sd, v, None, None)
    # nothing to do: no pointer is looked at
    assert lib.bgls_bb_verify_batch_combined(0, None, None, None, None, 0, None, 0, None, None, None) == 0
    assert lib.bgls_bb_verify_batch_combined_dev(1, None, None, None, None, 0, None, 0, None, None, None, None) == 0
    for call in (host, dev):
        # a NULL seed
        assert call(2, (U64 * 3)(0, 1, 2), 2, None) == ERR_ARG
        assert call(2, None, 1, None) == ERR_ARG
        # group_off not from 0, not ending at n, non-monotone
        assert call(2, (U64 * 3)(1, 1, 2), 2, seed) == ERR_ARG
        assert call(2, (U64 * 3)(0, 1, 1), 2, seed) == ERR_ARG
        assert call(2, (U64 * 3)(0, 1, 3), 2, seed) == ERR_ARG
        assert call(2, (U64 * 4)(0, 2, 1, 2), 3, seed) == ERR_ARG
        # NULL group_off with n_groups != 1
        assert call(2, None, 2, seed) == ERR_ARG
        assert call(2, None, 0, seed) == ERR_ARG
        # 2^28 items: the XOF length 16 n is a uint32
        assert call(1 << 28, None, 1, seed) == ERR_ARG
        # NULL arrays with n = 1, well-formed groups: still an argument error, before any device work
        assert call(1, None, 1, seed, None) == ERR_ARG
        assert call(1, (U64 * 2)(0, 1), 1, seed, None) == ERR_ARG
    assert lib.bgls_bb_verify_batch_combined(0, b, b, b, b, 1, None, 1, seed, None, None) == ERR_ARG          # NULL verdicts
    assert lib.bgls_bb_verify_batch_combined_dev(0, p, None, p, p, 1, None, 1, seed, v, None, None) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
sig = (ctypes.c_uint8 * 64)()
sc = (ctypes.c_uint8 * 32)()
key = (ctypes.c_uint8 * 256)()
seed = (ctypes.c_uint8 * 32)()
goff = (ctypes.c_uint64 * 2)(0, 1)
v = (ctypes.c_uint8 * 1)()
print(lib.bgls_bb_verify_batch_combined(0, sig, sc, key, sc, 1, None, 1, seed, v, None),
      lib.bgls_bb_verify_batch_combined_dev(0, ctypes.addressof(sig), ctypes.addressof(sc), ctypes.addressof(key), ctypes.addressof(sc), 1, goff, 1, seed, v,
                                            None, None))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2, r.stdout


def test_python_module_has_the_combined_forms():
    from bgls_amd import bbsigs
    for name in ("VerifyBatchCombined", "VerifyBatchLocated", "VerifyHashedBatchCombined", "VerifyHashedBatchLocated"):
        assert callable(getattr(bbsigs, name, None)), name


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "bbc.cpp"
    src.write_text('#include "bgls/bgls.hpp"\n'
                   "std::vector<bool> f(const curves::CurveSystem* c, const std::vector<curves::Point>& s, const std::vector<curves::Bytes>& r,\n"
                   "                    const std::vector<curves::Point>& u, const std::vector<curves::Point>& v, const std::vector<curves::Bytes>& m) {\n"
                   "  bool ok = false;\n"
                   "  std::vector<bool> groups = bgls::bb_verify_batch_combined(c, s, r, u, v, m, 64, curves::Bytes(32, 7), &ok);\n"
                   "  std::vector<bool> one = bgls::bb_verify_batch_combined(c, s, r, u, v, m);\n"
                   "  std::vector<bool> items = bgls::bb_verify_batch_located(c, s, r, u, v, m);\n"
                   "  return ok && !one.empty() && !groups.empty() ? items : bgls::bb_verify_batch_located(c, s, r, u, v, m, 16, curves::Bytes(32, 7));\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
