"""Builds tests/harness/libhost_harness_wirex.so (TEST-ONLY: the compressed wire formats on the carry-free limbs, wire_x.hpp, compiled
for the host with every column accumulation checked: wirex_host.cpp).  Used by tests/test_wirex_host.py, which builds it on first use."""
import glob, os, subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CLANGXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = os.path.join(HERE, "wirex_host.cpp")
SO = os.path.join(HERE, "libhost_harness_wirex.so")


def deps():
    return [SRC] + glob.glob(os.path.join(ROOT, "bgls_amd", "csrc", "*.hpp"))


def stale():
    return not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps())


def build(force=False, timeout=900):
    if not force and not stale():
        return SO
    tmp = SO + ".tmp%d" % os.getpid()
    subprocess.run([CLANGXX, "-std=c++17", "-O1", "-fPIC", "-shared", SRC, "-o", tmp], check=True, timeout=timeout)
    os.replace(tmp, SO)
    return SO


if __name__ == "__main__":
    print(build(force=True))
