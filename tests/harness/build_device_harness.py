"""Builds the TEST-ONLY device harness with the product Makefile's flags: tests/harness/libdevice_harness.so (device_harness.hip, the device
arithmetic and k_hash.hip's kernels behind batched C exports for the GPU tier, device_harness_points.hip, the point layer, and
device_harness_f12.hip, the cooperative Fp12 forms) and tests/harness/libdevice_harness_h2c.so (device_harness_h2c.hip: k_hash.hip's
alt-bn128 schedules over scripted digests -- it holds k_hash.hip's launchers a second time, so it is an object of its own).  The four
translation units are compiled in parallel, then each object is linked.  Used by tests/device_harness_lib.py and __graft_entry__.build()."""
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
SRCS_H2C = [os.path.join(HERE, "device_harness_h2c.hip")]
SO_H2C = os.path.join(HERE, "libdevice_harness_h2c.so")
OBJECTS = [(SO, SRCS), (SO_H2C, SRCS_H2C)]


def deps():
    return SRCS + SRCS_H2C + [os.path.join(HERE, f) for f in ("point_ops.hpp", "dev_bufs.hpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".hip", ".inc"))]


def stale():
    return any(not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps()) for so, _ in OBJECTS)


def build(force=False, timeout=900):
    """Both objects; returns the path of libdevice_harness.so (libdevice_harness_h2c.so: SO_H2C)."""
    if not force and not stale():
        return SO
    tmps = [so + ".tmp%d" % os.getpid() for so, _ in OBJECTS]
    try:
        with tempfile.TemporaryDirectory(prefix="bgls_dh_") as work:
            units = [src for _, srcs in OBJECTS for src in srcs]
            objs = [os.path.join(work, "unit%d.o" % k) for k in range(len(units))]

            def one(k):
                subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", CSRC, "-c", units[k], "-o", objs[k]],
                               check=True, timeout=timeout)

            with ThreadPoolExecutor(max_workers=len(units)) as ex:
                list(ex.map(one, range(len(units))))
            k = 0
            for tmp, (_, srcs) in zip(tmps, OBJECTS):
                subprocess.run([HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", tmp] + objs[k:k + len(srcs)], check=True, timeout=timeout)
                k += len(srcs)
        for tmp, (so, _) in zip(tmps, OBJECTS):
            os.replace(tmp, so)
    finally:
        for tmp in tmps:
            if os.path.exists(tmp):
                os.remove(tmp)
    return SO


if __name__ == "__main__":
    import time
    t0 = time.time()
    print(build(force=True))
    print(SO_H2C)
    print("compiled in %.0f s" % (time.time() - t0))
