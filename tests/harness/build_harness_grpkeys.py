"""Builds tests/harness/libhost_harness_grpkeys.so (TEST-ONLY: the selection arithmetic and the small / large work plan of the grouped
verification over a key set, grpkeys.hpp, compiled for the host: grpkeys_host.cpp).  Used by tests/test_grpkeys_host.py, which builds it
on first use."""
import os, subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "grpkeys_host.cpp")
SO = os.path.join(HERE, "libhost_harness_grpkeys.so")


def deps():
    return [SRC, os.path.join(ROOT, "bgls_amd", "csrc", "grpkeys.hpp"), os.path.join(ROOT, "bgls_amd", "csrc", "msggroup.hpp")]


def stale():
    return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps())


def build(force=False, timeout=300):
    if not force and not stale():
        return SO
    tmp = SO + ".tmp%d" % os.getpid()
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-fPIC", "-shared", SRC, "-o", tmp], check=True, timeout=timeout)
    os.replace(tmp, SO)
    return SO


if __name__ == "__main__":
    print(build(force=True))
