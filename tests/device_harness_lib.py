"""Loader of the test-only device harness (tests/harness/libdevice_harness.so, and libdevice_harness_h2c.so with the scripted-digest
alt-bn128 schedules) for the GPU-tier files: rebuilt (hipcc under a timeout) when any source is newer than it, loaded once per process,
argument types declared."""
import ctypes
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None
_LIB_H2C = None


def _builder():
    spec = importlib.util.spec_from_file_location("build_device_harness", os.path.join(ROOT, "tests", "harness", "build_device_harness.py"))
    bdh = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bdh)
    return bdh


def load():
    global _LIB
    if _LIB is None:
        lib = ctypes.CDLL(_builder().build(timeout=900))
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.dh_fp_op.argtypes = [i, i, sz, vp, vp, vp]
        lib.dh_f2_op.argtypes = [i, i, sz, vp, vp, vp]
        lib.dh_rx_sqrt.argtypes = [i, i, sz, vp, vp]
        lib.dh_rx_raw.argtypes = [i, i, i, sz, vp, vp, vp]
        lib.dh_bls_sw.argtypes = [sz, vp, i, vp, vp, vp]
        lib.dh_padd.argtypes = [i, i, sz, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.dh_pmul.argtypes = [i, i, sz, vp, vp, vp, vp, vp, vp]
        lib.dh_f12.argtypes = [i, i, i, i, sz, vp, vp, vp, i, i, vp, vp]
        lib.dh_f12_results.argtypes = [i, i, i]
        lib.dh_f12_slot_words.argtypes = [i, i]
        lib.dh_f12_half_stride.argtypes = [i]
        lib.dh_finalx.argtypes = [i, i, sz, i, vp, vp, vp, vp, vp]
        _LIB = lib
    return _LIB


def load_h2c():
    """libdevice_harness_h2c.so: dh_h2c_bn, kl::h2c_bn over scripted digests (tests/harness/device_harness_h2c.hip)"""
    global _LIB_H2C
    if _LIB_H2C is None:
        bdh = _builder()
        bdh.build(timeout=900)
        lib = ctypes.CDLL(bdh.SO_H2C)
        vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
        lib.dh_h2c_bn.argtypes = [sz, i, vp, vp, vp, vp, vp]
        _LIB_H2C = lib
    return _LIB_H2C
