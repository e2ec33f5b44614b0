#!/usr/bin/env python3
"""Throughput of bgls_verify_multi_hae_sets_dev (n_sets VerifyMultiSignatureWithHAE calls, one verdict each) against a loop of
bgls_verify_multi_hae over the first --single-cap sets of the same shape, with the batch's inputs resident on the device.

Shapes (sets x keys per set): 2^13 x 128, 2^10 x 1024, 2^16 x 16.  Keys of a set are a window of a pool of distinct keys; each set's
signature is AggregateSignaturesWithHAE's, made as (sum_i t_i sk_i) H(m_b).  Every verdict is checked.  Also times the BLAKE2Xb root of
one set on the device and on the host (bgls_hae_exponents_sets with bgls_set_hae_root_host_min at SIZE_MAX / 0), which sets the
default of that threshold.  Prints one JSON line: sets/s of both ways, us per set and per key, and the per-call stage times.
usage: python tools/gpu_multi_hae_sets.py [--curves 0,1] [--shapes 13x128,10x1024,16x16] [--steps 3] [--warmup 1] [--single-cap 2048]"""
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
SIZE_MAX = (1 << 64) - 1
HOST_MIN_DEFAULT = 2048
STAGES = ("hae_keys", "sum_points", "h2c", "miller", "epilogue", "final_exp")


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
    rnd = random.Random(3000 + cid)
    sks = [rnd.randrange(1, ORDER[cid]) for _ in range(POOL)]
    pool = (ctypes.c_uint8 * (POOL * g2b))()
    check(lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), POOL, pool), "scale_generator")
    # set b: pool keys (b + j) mod POOL, j < k
    t_pool = torch.frombuffer(bytearray(bytes(pool)), dtype=torch.uint8).to(dev).view(POOL, g2b)
    idx = ((torch.arange(ns, device=dev).view(ns, 1) + torch.arange(k, device=dev).view(1, k)) % POOL).reshape(-1)
    t_keys = t_pool[idx].contiguous()
    h_keys = bytes(t_keys.cpu().numpy().tobytes())
    t_exp = (ctypes.c_uint8 * (16 * ns * k))()
    check(lib.bgls_hae_exponents_sets(cid, B(h_keys), offs([k] * ns), ns, t_exp), "hae_exponents_sets")
    t_exp = bytes(t_exp)
    hidx = idx.cpu().tolist()
    agg = [sum(int.from_bytes(t_exp[16 * i:16 * i + 16], "big") * sks[hidx[i]] for i in range(b * k, (b + 1) * k)) % ORDER[cid] for b in range(ns)]
    msgs = rnd.randbytes(MSG * ns)
    sigs = (ctypes.c_uint8 * (ns * g1b))()
    check(lib.bgls_sign_batch(cid, B(b"".join(s.to_bytes(32, "big") for s in agg)), B(msgs), offs([MSG] * ns), ns, sigs), "sign_batch")
    t_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    t_sigs = torch.frombuffer(bytearray(bytes(sigs)), dtype=torch.uint8).to(dev)
    t_koff = torch.arange(ns + 1, dtype=torch.int64, device=dev) * k
    torch.cuda.synchronize()

    def sets_call():
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_verify_multi_hae_sets_dev(cid, t_sigs.data_ptr(), t_keys.data_ptr(), t_koff.data_ptr(), ns, k, t_msgs.data_ptr(), MSG, MSG, v,
                                                      None, None, None), "verify_multi_hae_sets_dev")
        if rc != ns or sum(v) != ns:
            raise RuntimeError("sets: %d of %d accepted" % (rc, ns))

    m1 = min(ns, cap)
    hs = bytes(sigs)

    def single_loop():
        for b in range(m1):
            rc = lib.bgls_verify_multi_hae(cid, B(hs[b * g1b:(b + 1) * g1b]), B(h_keys[b * k * g2b:(b + 1) * k * g2b]), k, B(msgs[b * MSG:(b + 1) * MSG]), MSG)
            if rc != 1:
                raise RuntimeError("single: set %d gave %d" % (b, rc))

    res = {"curve": "altbn128" if cid == 0 else "bls12", "sets": ns, "keys_per_set": k}
    for _ in range(warmup):
        sets_call()
    lib.bgls_profile_enable(1)
    t0 = time.perf_counter()
    for _ in range(steps):
        sets_call()
    dt = (time.perf_counter() - t0) / steps
    res["stage_ms"] = stage_times(lib, steps)
    lib.bgls_profile_enable(0)
    res["sets_ms_per_call"] = round(1e3 * dt, 3)
    res["sets_us_per_set"] = round(1e6 * dt / ns, 3)
    res["hae_keys_us_per_key"] = round(1e3 * res["stage_ms"].get("hae_keys", 0) / (ns * k), 4)
    single_loop()
    t0 = time.perf_counter()
    single_loop()
    res["single_us_per_set"] = round(1e6 * (time.perf_counter() - t0) / m1, 2)
    res["single_sets_timed"] = m1
    res["batch_vs_single"] = round(res["single_us_per_set"] / res["sets_us_per_set"], 2)
    return res


def root_costs(lib, cid, sizes):
    """ms of bgls_hae_exponents_sets on one set of k keys, every root on the device vs on the host"""
    fp = 32 if cid == 0 else 48
    kmax = max(sizes)
    keys = (ctypes.c_uint8 * (kmax * 4 * fp))()
    check(lib.bgls_scale_generator(cid, 2, B(b"".join((7 + i).to_bytes(32, "big") for i in range(kmax))), kmax, keys), "scale_generator")
    t = (ctypes.c_uint8 * (16 * kmax))()
    res = {}
    try:
        for k in sizes:
            for where, hm in (("device", SIZE_MAX), ("host", 0)):
                check(lib.bgls_set_hae_root_host_min(hm), "set_hae_root_host_min")
                check(lib.bgls_hae_exponents_sets(cid, keys, offs([k]), 1, t), "hae_exponents_sets")
                t0 = time.perf_counter()
                for _ in range(3):
                    check(lib.bgls_hae_exponents_sets(cid, keys, offs([k]), 1, t), "hae_exponents_sets")
                res["%s_%d" % (where, k)] = round(1e3 * (time.perf_counter() - t0) / 3, 3)
    finally:
        lib.bgls_set_hae_root_host_min(HOST_MIN_DEFAULT)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--shapes", default="13x128,10x1024,16x16")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--single-cap", type=int, default=2048)
    ap.add_argument("--root-sizes", default="256,1024,2048,4096,16384")
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs, roots = [], {}
    for c in a.curves.split(","):
        roots[c] = root_costs(lib, int(c), [int(x) for x in a.root_sizes.split(",")])
        print(json.dumps({"root_ms": roots[c], "curve": c}), file=sys.stderr, flush=True)
        for sh in a.shapes.split(","):
            l2, k = sh.split("x")
            recs.append(measure(lib, int(c), 1 << int(l2), int(k), a.steps, a.warmup, a.single_cap))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "gpu_multi_hae_sets", "root_ms": roots, "results": recs}))


if __name__ == "__main__":
    main()
