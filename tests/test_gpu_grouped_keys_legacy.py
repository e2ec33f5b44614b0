"""GPU tier: the grouped verification over a key set reads the set's sum-ready records, which only the lane-pair key sum does.  With that
kernel switched off (BGLS_LEGACY bit 8, which only libbgls_hip_legacy.so honours; the mask is read once per process, hence the child)
both forms refuse with BGLS_ERR_ARG before any device work, and the existing grouped call on the gathered keys still answers; the shipped
library ignores the bit and answers."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, sys
sys.path.insert(0, %r)
import torch
from bgls_amd import _lib
lib = _lib.load()
assert lib.bgls_init(0) == 0
cid, fp, n = 0, 32, 5
B = lambda b: (ctypes.c_uint8 * len(b)).from_buffer_copy(b)
sel = [0, 2, 4]
sks = [(1000 + i).to_bytes(32, "big") for i in range(n)]
keys = (ctypes.c_uint8 * (n * 4 * fp))()
assert lib.bgls_scale_generator(cid, 2, B(b"".join(sks)), n, keys) == 0
h = ctypes.c_uint64()
assert lib.bgls_keys_upload(cid, keys, n, (ctypes.c_int * 1)(0), 1, 0, ctypes.byref(h)) == 0
msgs = [b"m" * 8, b"q" * 8, b"m" * 8]
blob, off = B(b"".join(msgs)), (ctypes.c_uint64 * 4)(0, 8, 16, 24)
sigs = (ctypes.c_uint8 * (3 * 2 * fp))()
assert lib.bgls_sign_batch(cid, B(b"".join(sks[i] for i in sel)), blob, off, 3, sigs) == 0
sig = (ctypes.c_uint8 * (2 * fp))()
assert lib.bgls_aggregate_points(cid, 1, sigs, 3, sig) == 0
gathered = B(b"".join(bytes(keys)[i * 4 * fp:(i + 1) * 4 * fp] for i in sel))
row = (ctypes.c_uint8 * 4)(0b10101, 0, 0, 0)
dev = lambda b: torch.frombuffer(bytearray(bytes(b)), dtype=torch.uint8).to("cuda:0")
d_sig, d_row, d_msgs = dev(sig), dev(row), dev(blob)
d = ctypes.c_size_t(0)
torch.cuda.synchronize()
print("RESULT", lib.bgls_verify_aggregate_grouped_h(h, sig, row, 4, blob, off, 3, ctypes.byref(d), None),
      lib.bgls_verify_aggregate_grouped_keys_dev(h, d_sig.data_ptr(), d_row.data_ptr(), 4, d_msgs.data_ptr(), 8, 8, 3, ctypes.byref(d), None, None),
      lib.bgls_verify_aggregate_grouped(cid, sig, gathered, blob, off, 3, ctypes.byref(d), None), d.value)
"""


def run(env):
    e = dict(os.environ)
    e.pop("BGLS_LIB_VARIANT", None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [int(x) for x in [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1].split()[1:]]


def test_the_calls_refuse_when_the_lane_pair_key_sum_is_switched_off():
    assert os.path.exists(os.path.join(ROOT, "bgls_amd", "libbgls_hip_legacy.so")), "build it: make -C bgls_amd/csrc LEGACY=1 (or __graft_entry__.build())"
    assert run({"BGLS_LIB_VARIANT": "legacy", "BGLS_LEGACY": "8"}) == [-1, -1, 1, 2]


def test_the_shipped_library_ignores_the_bit():
    assert run({"BGLS_LEGACY": "8"}) == [1, 1, 1, 2]
