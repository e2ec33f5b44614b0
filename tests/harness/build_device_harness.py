"""Builds tests/harness/libdevice_harness.so (TEST-ONLY: device_harness.hip, the device arithmetic and k_hash.hip's kernels behind batched
C exports for the GPU tier) with the product Makefile's flags.  Used by tests/test_gpu_device_arith.py and __graft_entry__.build()."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "bgls_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRC = os.path.join(HERE, "device_harness.hip")
SO = os.path.join(HERE, "libdevice_harness.so")


def deps():
    return [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".inc"))]


def stale():
    return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps())


def build(force=False, timeout=900):
    if not force and not stale():
        return SO
    tmp = SO + ".tmp%d" % os.getpid()
    try:
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, SRC, "-o", tmp],
                       check=True, timeout=timeout)
        os.replace(tmp, SO)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return SO


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(build(force=True))
    print("compiled in %.0f s" % (time.time() - t0))
