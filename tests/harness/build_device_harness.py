"""Builds tests/harness/libdevice_harness.so (TEST-ONLY: device_harness.hip, the device arithmetic and k_hash.hip's kernels behind batched
C exports for the GPU tier, device_harness_points.hip, the point layer, and device_harness_f12.hip, the cooperative Fp12 forms) with the
product Makefile's flags: the three translation units are compiled in parallel and linked.  Used by tests/device_harness_lib.py and __graft_entry__.build()."""
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CSRC = os.path.join(ROOT, "bgls_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SRCS = [os.path.join(HERE, f) for f in ("device_harness.hip", "device_harness_points.hip", "device_harness_f12.hip")]
SO = os.path.join(HERE, "libdevice_harness.so")


def deps():
    return SRCS + [os.path.join(HERE, f) for f in ("point_ops.hpp", "dev_bufs.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".inc"))]


def stale():
    return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps())


def build(force=False, timeout=900):
    if not force and not stale():
        return SO
    tmp = SO + ".tmp%d" % os.getpid()
    try:
        with tempfile.TemporaryDirectory(prefix="bgls_dh_") as work:
            objs = [os.path.join(work, "unit%d.o" % k) for k in range(len(SRCS))]

            def one(k):
                subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", CSRC, "-c", SRCS[k], "-o", objs[k]],
                               check=True, timeout=timeout)

            with ThreadPoolExecutor(max_workers=len(SRCS)) as ex:
                list(ex.map(one, range(len(SRCS))))
            subprocess.run([HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", tmp] + objs, check=True, timeout=timeout)
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
