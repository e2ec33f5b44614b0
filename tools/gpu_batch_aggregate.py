#!/usr/bin/env python3
"""Throughput of bgls_verify_aggregate_batch_dev against the single-call forms, at the same shape (inputs resident on the device):

  batch    B instances of N signers per call (default 16 x 2^16), two batches in flight on two contexts from two host threads
  singles  B single N-signer verifications in flight on B contexts (bgls_miller_product_dev + bgls_final_verify_submit_dev), the way
           bench.py runs its 2^16 records
  big      one B*N-signer single verification per call (2^20 by default), two in flight on two contexts from two host threads

Every verdict is checked inside the timed loop.  Prints one JSON line: pairs/s of each form, the batch's rate relative to `big`, and the
per-call stage times (bgls_profile_*) of the batch and of the big single call, each measured with one call in flight.
usage: python tools/gpu_batch_aggregate.py [--curves 0,1] [--batch 16] [--log2n 16] [--steps 8] [--warmup 2]"""
import argparse
import ctypes
import json
import os
import random
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bgls_amd import _lib  # noqa: E402

ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
MSG = 64
STAGES = ("dup_check", "h2c", "scatter", "miller", "reduce", "epilogue", "final_exp")


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


def two_threads(lib, steps, body):
    """body(k) runs `steps` calls on context k; two host threads, one context each.  Returns the wall time."""
    err = []

    def run(k):
        try:
            check(lib.bgls_select_context(k), "select_context")
            for _ in range(steps):
                body(k)
        except Exception as e:          # reported by the main thread
            err.append(e)

    ts = [threading.Thread(target=run, args=(k,)) for k in (0, 1)]
    t0 = time.perf_counter()
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    dt = time.perf_counter() - t0
    if err:
        raise err[0]
    return dt


def measure(lib, cid, nb, n1, steps, warmup):
    fp = 32 if cid == 0 else 48
    g1b, g2b = 2 * fp, 4 * fp
    n = nb * n1
    dev = torch.device("cuda:0")
    rnd = random.Random(1000 + cid)
    sks = [rnd.randrange(1, ORDER[cid]) for _ in range(n)]
    kb = B(b"".join(s.to_bytes(32, "big") for s in sks))
    msgs = rnd.randbytes(MSG * n)
    keys = (ctypes.c_uint8 * (n * g2b))()
    check(lib.bgls_scale_generator(cid, 2, kb, n, keys), "scale_generator")
    sigs = (ctypes.c_uint8 * (n * g1b))()
    check(lib.bgls_sign_batch(cid, kb, B(msgs), offs([MSG] * n), n, sigs), "sign_batch")
    aggs = (ctypes.c_uint8 * (nb * g1b))()
    check(lib.bgls_aggregate_sets(cid, 1, sigs, offs([n1] * nb), nb, aggs), "aggregate_sets")
    agg_all = (ctypes.c_uint8 * g1b)()
    check(lib.bgls_aggregate_points(cid, 1, aggs, nb, agg_all), "aggregate_points")
    t_keys = torch.frombuffer(bytearray(bytes(keys)), dtype=torch.uint8).to(dev)
    t_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    t_aggs = torch.frombuffer(bytearray(bytes(aggs)), dtype=torch.uint8).to(dev)
    t_all = torch.frombuffer(bytearray(bytes(agg_all)), dtype=torch.uint8).to(dev)
    torch.cuda.synchronize()
    inst_off = offs([n1] * nb)

    def batch_call(k):
        v = (ctypes.c_uint8 * nb)()
        rc = check(lib.bgls_verify_aggregate_batch_dev(cid, t_aggs.data_ptr(), t_keys.data_ptr(), inst_off, nb, t_msgs.data_ptr(), MSG, MSG, 0, v, None,
                                                       None), "verify_aggregate_batch_dev")
        if rc != nb or any(x != 1 for x in v):
            raise RuntimeError("batch: %d of %d instances accepted" % (rc, nb))

    parts = [torch.zeros(12 * fp, dtype=torch.uint8, device=dev) for _ in range(max(nb, 2))]
    flags = [torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(max(nb, 2))]
    streams = [torch.cuda.Stream(device=dev) for _ in range(max(nb, 2))]

    def big_call(k):
        with torch.cuda.stream(streams[k]):
            flags[k].zero_()
        h = streams[k].cuda_stream
        check(lib.bgls_miller_product_dev(cid, t_all.data_ptr(), t_keys.data_ptr(), t_msgs.data_ptr(), MSG, MSG, n, 1, parts[k].data_ptr(),
                                          flags[k].data_ptr(), h), "miller_product_dev")
        if check(lib.bgls_final_verify_dev(cid, parts[k].data_ptr(), 1, flags[k].data_ptr(), h), "final_verify_dev") != 1:
            raise RuntimeError("single 2^%d call rejected" % (n.bit_length() - 1))

    def singles_step():
        for k in range(nb):
            check(lib.bgls_select_context(k), "select_context")
            with torch.cuda.stream(streams[k]):
                flags[k].zero_()
            h = streams[k].cuda_stream
            check(lib.bgls_miller_product_dev(cid, t_aggs.data_ptr() + k * g1b, t_keys.data_ptr() + k * n1 * g2b, t_msgs.data_ptr() + k * n1 * MSG, MSG, MSG,
                                              n1, 1, parts[k].data_ptr(), flags[k].data_ptr(), h), "miller_product_dev")
            check(lib.bgls_final_verify_submit_dev(cid, parts[k].data_ptr(), 1, flags[k].data_ptr(), h), "final_verify_submit_dev")
        for k in range(nb):
            check(lib.bgls_select_context(k), "select_context")
            if check(lib.bgls_final_verify_collect(cid), "final_verify_collect") != 1:
                raise RuntimeError("single call %d rejected" % k)
        check(lib.bgls_select_context(0), "select_context")

    # stage times with one call in flight (the lone launch shapes: throughput mode 2)
    check(lib.bgls_set_throughput_mode(2), "set_throughput_mode")
    check(lib.bgls_select_context(0), "select_context")
    for _ in range(max(1, warmup)):
        batch_call(0)
        big_call(0)
    lib.bgls_profile_enable(1)
    for _ in range(steps):
        batch_call(0)
    st_batch = stage_times(lib, steps)
    lib.bgls_profile_enable(1)
    for _ in range(steps):
        big_call(0)
    st_big = stage_times(lib, steps)
    lib.bgls_profile_enable(0)
    # throughput: several calls in flight
    check(lib.bgls_set_throughput_mode(1), "set_throughput_mode")
    two_threads(lib, 1, batch_call)
    dt_batch = two_threads(lib, steps, batch_call)
    two_threads(lib, 1, big_call)
    dt_big = two_threads(lib, steps, big_call)
    singles_step()
    t0 = time.perf_counter()
    for _ in range(steps):
        singles_step()
    dt_singles = time.perf_counter() - t0
    check(lib.bgls_set_throughput_mode(0), "set_throughput_mode")
    r_batch = 2 * steps * n / dt_batch
    r_big = 2 * steps * n / dt_big
    r_singles = steps * n / dt_singles
    return {"curve": "altbn128" if cid == 0 else "bls12", "instances": nb, "signers_per_instance": n1,
            "batch_pairs_per_s": round(r_batch), "singles_in_flight_pairs_per_s": round(r_singles), "big_single_pairs_per_s": round(r_big),
            "batch_vs_big": round(r_batch / r_big, 4), "singles_vs_big": round(r_singles / r_big, 4),
            "stage_ms_batch": st_batch, "stage_ms_big_single": st_big}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--log2n", type=int, default=16)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = [measure(lib, int(c), a.batch, 1 << a.log2n, a.steps, a.warmup) for c in a.curves.split(",")]
    print(json.dumps({"tool": "gpu_batch_aggregate", "results": recs}))


if __name__ == "__main__":
    main()
