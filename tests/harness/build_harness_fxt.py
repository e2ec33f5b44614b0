"""Builds tests/harness/libhost_harness_fxt.so (TEST-ONLY: the throughput final exponentiation of finalxt.hpp walked on the host,
host_harness_fxt.cpp).  Used by tests/test_fxt_host.py and __graft_entry__.build()."""
import os, subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "host_harness_fxt.cpp")
SO = os.path.join(HERE, "libhost_harness_fxt.so")


def deps():
    csrc = os.path.join(ROOT, "bgls_amd", "csrc")
    return [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]


def stale():
    return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps())


def build(force=False, timeout=900):
    if not force and not stale():
        return SO
    tmp = SO + ".tmp%d" % os.getpid()
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-fPIC", "-pthread", "-shared", SRC, "-o", tmp], check=True, timeout=timeout)
    os.replace(tmp, SO)
    return SO


if __name__ == "__main__":
    print(build(force=True))
