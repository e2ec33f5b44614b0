"""CPU tier: the batched Boneh-Boyen verification is exported with the signatures of include/bgls_hip.h, refuses without a usable GPU
with BGLS_ERR_NO_DEVICE (no host fallback), checks its arguments before it needs a device, and has its Python and C++ mirrors."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NO_DEVICE = -1, -4


def test_bb_symbols_are_exported():
    from bgls_amd import _lib
    lib = _lib.load()
    for name in ("bgls_bb_verify_batch", "bgls_bb_verify_batch_dev"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.bgls_abi_version() == 2


def test_argument_checks_need_no_device():
    from bgls_amd import _lib
    lib = _lib.load()
    v = (ctypes.c_uint8 * 1)()
    b = (ctypes.c_uint8 * 256)()
    assert lib.bgls_bb_verify_batch(0, None, None, None, None, 0, None, None) == 0
    assert lib.bgls_bb_verify_batch_dev(1, None, None, None, None, 0, None, None, None) == 0
    assert lib.bgls_bb_verify_batch(0, None, b, b, b, 1, v, None) == ERR_ARG
    assert lib.bgls_bb_verify_batch(1, b, b, b, b, 1, None, None) == ERR_ARG
    assert lib.bgls_bb_verify_batch(0, b, b, b, b, 1 << 30, v, None) == ERR_ARG
    assert lib.bgls_bb_verify_batch_dev(0, ctypes.addressof(b), None, ctypes.addressof(b), ctypes.addressof(b), 1, v, None, None) == ERR_ARG


_NO_DEVICE = r"""
import ctypes, sys
sys.path.insert(0, %r)
from bgls_amd import _lib
lib = _lib.load()
sig = (ctypes.c_uint8 * 64)()
sc = (ctypes.c_uint8 * 32)()
key = (ctypes.c_uint8 * 256)()
v = (ctypes.c_uint8 * 1)()
print(lib.bgls_bb_verify_batch(0, sig, sc, key, sc, 1, v, None),
      lib.bgls_bb_verify_batch_dev(0, ctypes.addressof(sig), ctypes.addressof(sc), ctypes.addressof(key), ctypes.addressof(sc), 1, v, None, None))
"""


def test_no_device_means_an_error_not_a_fallback():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", _NO_DEVICE % ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == [str(ERR_NO_DEVICE)] * 2, r.stdout


def test_python_module_mirrors_the_reference_names():
    from bgls_amd import bbsigs
    for name in ("Privkey", "Pubkey", "Signature", "KeyGen", "LoadPublicKey", "Sign", "SignHashed", "SignCustHash", "Verify", "VerifyHashed",
                 "VerifyCustHash", "VerifyBatch", "VerifyHashedBatch", "SignBatch"):
        assert hasattr(bbsigs, name), name
    # blake2b256 (bbsigs/hashedbbsigs.go:34-39): Sum256 of the message, reduced modulo the order
    import hashlib
    q = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    for m in (b"", b"a", bytes(128), bytes(129)):
        assert bbsigs.blake2b256(m, q) == int.from_bytes(hashlib.blake2b(m, digest_size=32).digest(), "big") % q
    assert bbsigs.blake2b256(b"", q) == int("0e5751c026e543b2e8ab2eb06099daa1d1e5df47778f7787faab45cdf12fe3a8", 16) % q


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / "bb.cpp"
    src.write_text('#include "bgls/bgls.hpp"\n'
                   "std::vector<bool> f(const curves::CurveSystem* c, const std::vector<curves::Point>& s, const std::vector<curves::Bytes>& r,\n"
                   "                    const std::vector<curves::Point>& u, const std::vector<curves::Point>& v, const std::vector<curves::Bytes>& m) {\n"
                   "  return bgls::bb_verify_batch(c, s, r, u, v, m);\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
