#!/usr/bin/env python3
"""Throughput of bgls_verify_multi_sets_dev (n_sets independent multi-signatures, one verdict each) against two other ways of
running the same sets, with inputs resident on the device:

  sets    one bgls_verify_multi_sets_dev call per step
  padded  (a) bgls_aggregate_sets (the key sums), then bgls_verify_aggregate_batch_dev with one-pair instances: k_miller_x60 with every
          set padded to a whole six-pairing group
  multi8  (b) bgls_verify_multi_submit_dev, one set per call, eight contexts in flight (the first --multi8-cap sets of the shape)

Shapes (sets x keys per set): 2^16 x 1 (batched single signatures), 2^16 x 128, 2^12 x 1024.  Keys of a set are a window of a pool
of distinct keys; each set's signature is made with the sum of its secret keys.  Every verdict is checked.  Prints one JSON line:
sets/s of each way and the per-call stage times (bgls_profile_*) of `sets` and `padded`, one call in flight.
usage: python tools/gpu_multi_sets.py [--curves 0,1] [--shapes 16x1,16x128,12x1024] [--steps 3] [--warmup 1] [--multi8-cap 4096]"""
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
STAGES = ("sum_points", "h2c", "scatter", "miller", "reduce", "epilogue", "final_exp")


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


def measure(lib, cid, ns, k, steps, warmup, cap):
    fp = 32 if cid == 0 else 48
    g1b, g2b = 2 * fp, 4 * fp
    dev = torch.device("cuda:0")
    rnd = random.Random(2000 + cid)
    sks = [rnd.randrange(1, ORDER[cid]) for _ in range(POOL)]
    pool = (ctypes.c_uint8 * (POOL * g2b))()
    check(lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), POOL, pool), "scale_generator")
    # set b: pool keys (b + j) mod POOL, j < k; its signature with the sum of their secret keys
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
    h_keys = t_keys.cpu().numpy()
    set_off = offs([k] * ns)
    one_off = offs([1] * ns)
    apks = (ctypes.c_uint8 * (ns * g2b))()
    t_apks = torch.zeros(ns * g2b, dtype=torch.uint8, device=dev)

    def sets_call():
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_verify_multi_sets_dev(cid, t_sigs.data_ptr(), t_keys.data_ptr(), t_koff.data_ptr(), ns, k, t_msgs.data_ptr(), MSG, MSG, v, None,
                                                  None), "verify_multi_sets_dev")
        if rc != ns:
            raise RuntimeError("sets: %d of %d accepted" % (rc, ns))

    def padded_call():
        check(lib.bgls_aggregate_sets(cid, 2, h_keys.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), set_off, ns, apks), "aggregate_sets")
        t_apks.copy_(torch.frombuffer(bytearray(bytes(apks)), dtype=torch.uint8))
        torch.cuda.synchronize()
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_verify_aggregate_batch_dev(cid, t_sigs.data_ptr(), t_apks.data_ptr(), one_off, ns, t_msgs.data_ptr(), MSG, MSG, 1, v, None, None),
                   "verify_aggregate_batch_dev")
        if rc != ns:
            raise RuntimeError("padded: %d of %d accepted" % (rc, ns))

    m8 = min(ns, cap)

    def multi8_run():
        inflight = []
        for b in range(m8):
            ctx = b % 8
            if len(inflight) == 8:
                c0 = inflight.pop(0)
                check(lib.bgls_select_context(c0), "select_context")
                if check(lib.bgls_final_verify_collect(cid), "final_verify_collect") != 1:
                    raise RuntimeError("multi8: a set was rejected")
            check(lib.bgls_select_context(ctx), "select_context")
            check(lib.bgls_verify_multi_submit_dev(cid, t_sigs.data_ptr() + b * g1b, t_keys.data_ptr() + b * k * g2b, k, t_msgs.data_ptr() + b * MSG, MSG,
                                                   None), "verify_multi_submit_dev")
            inflight.append(ctx)
        for c0 in inflight:
            check(lib.bgls_select_context(c0), "select_context")
            if check(lib.bgls_final_verify_collect(cid), "final_verify_collect") != 1:
                raise RuntimeError("multi8: a set was rejected")
        check(lib.bgls_select_context(0), "select_context")

    res = {"curve": "altbn128" if cid == 0 else "bls12", "sets": ns, "keys_per_set": k}
    for name, fn in (("sets", sets_call), ("padded", padded_call)):
        for _ in range(warmup):
            fn()
        lib.bgls_profile_enable(1)
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        dt = time.perf_counter() - t0
        res[name + "_sets_per_s"] = round(steps * ns / dt)
        res["stage_ms_" + name] = stage_times(lib, steps)
        lib.bgls_profile_enable(0)
    multi8_run()
    t0 = time.perf_counter()
    multi8_run()
    res["multi8_sets_per_s"] = round(m8 / (time.perf_counter() - t0))
    res["multi8_sets_timed"] = m8
    res["sets_vs_padded"] = round(res["sets_sets_per_s"] / res["padded_sets_per_s"], 3)
    res["sets_vs_multi8"] = round(res["sets_sets_per_s"] / res["multi8_sets_per_s"], 3)
    mp, ms = res["stage_ms_padded"].get("miller"), res["stage_ms_sets"].get("miller")
    if mp and ms:
        res["miller_us_per_set"] = {"sets": round(1e3 * ms / ns, 4), "padded": round(1e3 * mp / ns, 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--shapes", default="16x1,16x128,12x1024")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--multi8-cap", type=int, default=4096)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        for sh in a.shapes.split(","):
            l2, k = sh.split("x")
            recs.append(measure(lib, int(c), 1 << int(l2), int(k), a.steps, a.warmup, a.multi8_cap))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "gpu_multi_sets", "results": recs}))


if __name__ == "__main__":
    main()
