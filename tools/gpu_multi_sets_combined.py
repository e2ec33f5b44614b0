#!/usr/bin/env python3
"""Throughput of bgls_verify_multi_sets_combined_dev (one combined check per group of sets) against bgls_verify_multi_sets_dev (one
verdict and one final exponentiation per set) on the same device-resident inputs, in the same run:

  one      the combined call with one group over all sets (group_off = NULL)
  g64      the combined call with groups of 64 consecutive sets
  per_set  bgls_verify_multi_sets_dev

Shapes (sets x keys per set): 2^16 x 1 and 2^16 x 128; inputs as tools/gpu_multi_sets.py makes them (keys of a set are a window of a
pool of distinct keys, each set's signature is made with the sum of its secret keys).  Every verdict is checked.  Each way is warmed
up, then timed over --steps calls, one call in flight.  Prints one JSON line: sets/s of each way and its per-call stage times.
usage: python tools/gpu_multi_sets_combined.py [--curves 0,1] [--shapes 16x1,16x128] [--steps 5] [--warmup 2]"""
import argparse
import ctypes
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bgls_amd import _lib  # noqa: E402

ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
MSG = 32
POOL = 4096
STAGES = ("sum_points", "h2c", "rlc", "scatter", "miller", "reduce", "epilogue", "final_exp")


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %d %s" % (what, rc, _lib.last_error()))
    return rc


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def offs(counts):
    o = (ctypes.c_uint64 * (len(counts) + 1))()
    for i, c in enumerate(counts):
        o[i + 1] = o[i] + c
    return o


def stage_times(lib, calls):
    res = {}
    for s in STAGES:
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        check(lib.bgls_profile_get(s.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "profile_get")
        if cnt.value:
            res[s] = round(ms.value / calls, 4)
    return res


def measure(lib, cid, ns, k, steps, warmup):
    fp = 32 if cid == 0 else 48
    g1b, g2b = 2 * fp, 4 * fp
    dev = torch.device("cuda:0")
    rnd = random.Random(2000 + cid)
    sks = [rnd.randrange(1, ORDER[cid]) for _ in range(POOL)]
    pool = (ctypes.c_uint8 * (POOL * g2b))()
    check(lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), POOL, pool), "scale_generator")
    pre = [0]
    for i in range(POOL + k):
        pre.append(pre[-1] + sks[i % POOL])
    ssum = [(pre[b % POOL + k] - pre[b % POOL]) % ORDER[cid] for b in range(ns)]
    msgs = rnd.randbytes(MSG * ns)
    sigs = (ctypes.c_uint8 * (ns * g1b))()
    check(lib.bgls_sign_batch(cid, B(b"".join(s.to_bytes(32, "big") for s in ssum)), B(msgs), offs([MSG] * ns), ns, sigs), "sign_batch")
    t_pool = torch.frombuffer(bytearray(bytes(pool)), dtype=torch.uint8).to(dev).view(POOL, g2b)
    idx = (torch.arange(ns, device=dev).view(ns, 1) + torch.arange(k, device=dev).view(1, k)) % POOL
    t_keys = t_pool[idx.reshape(-1)].contiguous()
    t_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    t_sigs = torch.frombuffer(bytearray(bytes(sigs)), dtype=torch.uint8).to(dev)
    t_koff = torch.arange(ns + 1, dtype=torch.int64, device=dev) * k
    torch.cuda.synchronize()
    g64 = offs([64] * (ns // 64) + ([ns % 64] if ns % 64 else []))
    n64 = len(g64) - 1

    def combined(goff, ng):
        def call():
            v = (ctypes.c_uint8 * ng)()
            rc = check(lib.bgls_verify_multi_sets_combined_dev(cid, t_sigs.data_ptr(), t_keys.data_ptr(), t_koff.data_ptr(), ns, k, t_msgs.data_ptr(), MSG, MSG,
                                                               goff, ng, B(os.urandom(32)), v, None, None), "verify_multi_sets_combined_dev")
            if rc != ng:
                raise RuntimeError("combined: %d of %d groups accepted" % (rc, ng))
        return call

    def per_set():
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_verify_multi_sets_dev(cid, t_sigs.data_ptr(), t_keys.data_ptr(), t_koff.data_ptr(), ns, k, t_msgs.data_ptr(), MSG, MSG, v, None,
                                                  None), "verify_multi_sets_dev")
        if rc != ns:
            raise RuntimeError("per_set: %d of %d accepted" % (rc, ns))

    res = {"curve": "altbn128" if cid == 0 else "bls12", "sets": ns, "keys_per_set": k}
    for name, fn in (("one", combined(None, 1)), ("g64", combined(g64, n64)), ("per_set", per_set)):
        for _ in range(warmup):
            fn()
        lib.bgls_profile_enable(1)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        dt = time.perf_counter() - t0
        res[name + "_sets_per_s"] = round(steps * ns / dt)
        res[name + "_ms_per_call"] = round(1e3 * dt / steps, 3)
        res["stage_ms_" + name] = stage_times(lib, steps)
        lib.bgls_profile_enable(0)
    res["one_vs_per_set"] = round(res["one_sets_per_s"] / res["per_set_sets_per_s"], 3)
    res["g64_vs_per_set"] = round(res["g64_sets_per_s"] / res["per_set_sets_per_s"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--shapes", default="16x1,16x128")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        for sh in a.shapes.split(","):
            l2, k = sh.split("x")
            recs.append(measure(lib, int(c), 1 << int(l2), int(k), a.steps, a.warmup))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "gpu_multi_sets_combined", "results": recs}))


if __name__ == "__main__":
    main()
