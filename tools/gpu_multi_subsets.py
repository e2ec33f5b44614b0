#!/usr/bin/env python3
"""Throughput of bgls_verify_multi_subsets_keys_dev (n_sets multi-signatures whose signers are bitmap rows over ONE resident key set)
against the way such sets were verified before it, on the same machine in the same session, inputs resident on the device:

  subsets  one bgls_verify_multi_subsets_keys_dev call per step: the rows, nothing of a key
  gather   the selected keys gathered as wire bytes on the device (outside the timed region: the baseline is not charged for the
           gather or its upload) and handed to bgls_verify_multi_sets_dev

Shapes (keys x sets): 2^12 x 2^12 and 2^20 x 64, at participation 1 %, 50 % and 99 % (each key of each row drawn independently).  Secret
keys are small (below 2^31) so that a set's secret sum is an exact integer dot product; each set's signature is made with that sum.
Every verdict is checked.  Prints one JSON line: per shape and participation the median / min / max seconds of the repeated steps, sets/s
and signers/s of both ways, their ratio, and the key-sum stage ("sum_points", "sum_main": bgls_profile_*) per call of both.
usage: python tools/gpu_multi_subsets.py [--curves 0,1] [--shapes 12x12,20x6] [--parts 0.01,0.5,0.99] [--steps 5] [--warmup 1]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgls_amd import _lib  # noqa: E402

ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
MSG = 32
STAGES = ("sum_points", "sum_main", "h2c", "miller", "epilogue", "final_exp")


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


def timed(lib, fns, steps, warmup):
    """the ways alternate step by step with the stage timers off (host clock around calls that end in a synchronise); the stage times come
    from further steps of each way with the timers on"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    ts = [[] for _ in fns]
    for _ in range(steps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    stages = []
    for fn in fns:
        lib.bgls_profile_enable(1)
        for _ in range(steps):
            fn()
        stages.append(stage_times(lib, steps))
        lib.bgls_profile_enable(0)
    return ts, stages


def key_set(lib, cid, n, seed):
    fp = 32 if cid == 0 else 48
    rng = np.random.default_rng(seed)
    sks = rng.integers(1, 1 << 31, size=n, dtype=np.int64)
    raw = b"".join(int(s).to_bytes(32, "big") for s in sks)
    keys = (ctypes.c_uint8 * (n * 4 * fp))()
    check(lib.bgls_scale_generator(cid, 2, B(raw), n, keys), "scale_generator")
    h = ctypes.c_uint64()
    devs = (ctypes.c_int * 1)(0)
    check(lib.bgls_keys_upload(cid, keys, n, devs, 1, 0, ctypes.byref(h)), "keys_upload")
    t_keys = torch.frombuffer(bytearray(bytes(keys)), dtype=torch.uint8).to(torch.device("cuda:0")).view(n, 4 * fp)
    return sks, h.value, t_keys


def measure(lib, cid, n, ns, part, sks, h, t_keys, steps, warmup):
    fp = 32 if cid == 0 else 48
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(int(part * 1000) + 7 * cid + n)
    sel = rng.random((ns, n)) < part
    counts = sel.sum(axis=1)
    ssum = [int(s) % ORDER[cid] for s in sel.astype(np.int64) @ sks]
    msgs = rng.bytes(MSG * ns)
    sigs = (ctypes.c_uint8 * (ns * 2 * fp))()
    check(lib.bgls_sign_batch(cid, B(b"".join((s or 1).to_bytes(32, "big") for s in ssum)), B(msgs), offs([MSG] * ns), ns, sigs), "sign_batch")
    sigs = bytearray(bytes(sigs))
    for b in range(ns):
        if ssum[b] == 0:                                   # an empty row: the point at infinity
            sigs[b * 2 * fp:(b + 1) * 2 * fp] = bytes(2 * fp)
    stride = (n + 31) // 32 * 4
    rows = np.zeros((ns, stride), dtype=np.uint8)
    rows[:, :(n + 7) // 8] = np.packbits(sel, axis=1, bitorder="little")
    t_rows = torch.from_numpy(rows).to(dev)
    t_sigs = torch.frombuffer(sigs, dtype=torch.uint8).to(dev)
    t_msgs = torch.frombuffer(bytearray(msgs), dtype=torch.uint8).to(dev)
    idx = torch.from_numpy(np.nonzero(sel.reshape(-1))[0] % n).to(dev)
    t_gath = t_keys[idx].contiguous()                      # the baseline's input: the selected keys as wire bytes, set after set
    t_koff = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)
    torch.cuda.synchronize()
    max_set = int(counts.max())

    def subsets_call():
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_verify_multi_subsets_keys_dev(h, t_sigs.data_ptr(), t_rows.data_ptr(), stride, ns, t_msgs.data_ptr(), MSG, MSG, v, None, None, None),
                   "verify_multi_subsets_keys_dev")
        if rc != ns or sum(v) != ns:
            raise RuntimeError("subsets: %d of %d accepted" % (rc, ns))

    def gather_call():
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_verify_multi_sets_dev(cid, t_sigs.data_ptr(), t_gath.data_ptr(), t_koff.data_ptr(), ns, max_set, t_msgs.data_ptr(), MSG, MSG, v, None,
                                                  None), "verify_multi_sets_dev")
        if rc != ns or sum(v) != ns:
            raise RuntimeError("gather: %d of %d accepted" % (rc, ns))

    res = {"curve": "altbn128" if cid == 0 else "bls12", "keys": n, "sets": ns, "participation": part, "signers": int(counts.sum())}
    all_ts, all_stages = timed(lib, (subsets_call, gather_call), steps, warmup)
    for name, ts, stages in zip(("subsets", "gather"), all_ts, all_stages):
        med = statistics.median(ts)
        res[name] = {"s_median": round(med, 6), "s_min": round(min(ts), 6), "s_max": round(max(ts), 6), "sets_per_s": round(ns / med),
                     "signers_per_s": round(int(counts.sum()) / med), "stage_ms": stages}
    res["subsets_vs_gather"] = round(res["gather"]["s_median"] / res["subsets"]["s_median"], 3)
    del t_gath, idx
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--shapes", default="12x12,20x6")
    ap.add_argument("--parts", default="0.01,0.5,0.99")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        for sh in a.shapes.split(","):
            lk, ls = sh.split("x")
            n, ns = 1 << int(lk), 1 << int(ls)
            sks, h, t_keys = key_set(lib, int(c), n, 3000 + int(c))
            for p in a.parts.split(","):
                recs.append(measure(lib, int(c), n, ns, float(p), sks, h, t_keys, a.steps, a.warmup))
                print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            check(lib.bgls_keys_free(h), "keys_free")
            del t_keys
    print(json.dumps({"tool": "gpu_multi_subsets", "results": recs}))


if __name__ == "__main__":
    main()
