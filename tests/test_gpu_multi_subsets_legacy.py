"""GPU tier: the subset calls read a key set's sum-ready records, which only the lane-pair key sum does.  With that kernel switched off
(BGLS_LEGACY bit 8, which only libbgls_hip_legacy.so honours; the mask is read once per process, hence the child) every subset call
refuses with BGLS_ERR_ARG before any device work, and the whole-set calls on the same handle go on working; the shipped library ignores
the bit and answers."""
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
sks = b"".join((1000 + i).to_bytes(32, "big") for i in range(n))
keys = (ctypes.c_uint8 * (n * 4 * fp))()
assert lib.bgls_scale_generator(cid, 2, (ctypes.c_uint8 * len(sks)).from_buffer_copy(sks), n, keys) == 0
h = ctypes.c_uint64()
assert lib.bgls_keys_upload(cid, keys, n, (ctypes.c_int * 1)(0), 1, 0, ctypes.byref(h)) == 0
rows = (ctypes.c_uint8 * 4)(0b10101, 0, 0, 0)
out = (ctypes.c_uint8 * (4 * fp))()
sig = (ctypes.c_uint8 * (2 * fp))()
msg = (ctypes.c_uint8 * 8)()
off = (ctypes.c_uint64 * 2)(0, 8)
v = (ctypes.c_uint8 * 1)()
d = torch.zeros(256, dtype=torch.uint8, device="cuda:0")       # device form: an infinity signature, an empty row, a zero message
torch.cuda.synchronize()
print("RESULT", lib.bgls_aggregate_subsets_h(h, rows, 4, 1, out),
      lib.bgls_verify_multi_subsets_h(h, sig, rows, 4, 1, msg, off, v, None, None),
      lib.bgls_verify_multi_subsets_keys_dev(h, d.data_ptr(), d.data_ptr(), 4, 1, d.data_ptr(), 8, 8, v, None, None, None),
      lib.bgls_verify_multi_h(h, sig, msg, 8))
"""


def run(env):
    e = dict(os.environ)
    e.pop("BGLS_LIB_VARIANT", None)
    e.update(env)
    p = subprocess.run([sys.executable, "-c", CHILD % ROOT], capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return [int(x) for x in [l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1].split()[1:]]


def test_subset_calls_refuse_when_the_lane_pair_key_sum_is_switched_off():
    assert os.path.exists(os.path.join(ROOT, "bgls_amd", "libbgls_hip_legacy.so")), "build it: make -C bgls_amd/csrc LEGACY=1 (or __graft_entry__.build())"
    assert run({"BGLS_LIB_VARIANT": "legacy", "BGLS_LEGACY": "8"}) == [-1, -1, -1, 0]


def test_the_shipped_library_ignores_the_bit():
    # the key sums answer; the infinity signature is not the subset's, is the empty row's (device form), is not the whole set's
    assert run({"BGLS_LEGACY": "8"}) == [0, 0, 1, 0]
