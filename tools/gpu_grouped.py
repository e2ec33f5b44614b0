#!/usr/bin/env python3
"""Time of bgls_verify_aggregate_grouped_dev (one hash and one pairing per DISTINCT message, the keys of a message's signers summed first)
against the way such an instance was verified before it, on the same machine in the same session, inputs resident on the device:

  grouped   one bgls_verify_aggregate_grouped_dev call per step
  baseline  bgls_miller_product_dev(check_duplicates = 0) + bgls_final_verify_dev on the same keys and messages: n hashes, n + 1 Miller loops

n signers over d distinct 32-byte messages, the signers of a message scattered over the key array (a random assignment).  Even shapes:
d = 1, 64, n / 16, n / 4, n / 2, n with the signers spread evenly; skewed shapes ("skew"): one message signed by n / 2 signers, the rest
spread over d - 1 messages, at d = 64 and d = n / 4.  Secret keys are small (below 2^31) so that a group's secret sum is an exact integer;
the aggregate signature is the sum of the d group signatures.  Every verdict is checked (1, and n_groups = d).  The two ways alternate step
by step.  Prints one JSON line: per curve, n and shape the median / min seconds of both ways, their ratio, and the stage times per call
("group", "sum_points", "sum_main", "h2c", "miller", "final_exp": bgls_profile_*) of both.
usage: python tools/gpu_grouped.py [--curves 0,1] [--logn 16,20] [--steps 5] [--warmup 1] [--shapes even,skew]"""
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
STAGES = ("group", "sum_points", "sum_main", "h2c", "miller", "reduce", "final_exp")


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %d %s" % (what, rc, _lib.last_error()))
    return rc


def as_buf(a):
    return (ctypes.c_uint8 * max(1, a.size)).from_buffer_copy(a.tobytes() if a.size else b"\0")


def offs(n, step):
    return (ctypes.c_uint64 * (n + 1))(*range(0, step * (n + 1), step))


def be32(values):
    """non-negative integers below 2^63 as 32-byte big-endian scalars, one row each"""
    out = np.zeros((len(values), 32), dtype=np.uint8)
    out[:, 24:] = np.asarray(values, dtype=">u8").view(np.uint8).reshape(-1, 8)
    return out


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


def signers(lib, cid, n, seed):
    fp = 32 if cid == 0 else 48
    rng = np.random.default_rng(seed)
    sks = rng.integers(1, 1 << 31, size=n, dtype=np.int64)
    keys = (ctypes.c_uint8 * (n * 4 * fp))()
    check(lib.bgls_scale_generator(cid, 2, as_buf(be32(sks)), n, keys), "scale_generator")
    t_keys = torch.frombuffer(bytearray(bytes(keys)), dtype=torch.uint8).to(torch.device("cuda:0"))
    return sks, t_keys


def assignment(rng, n, d, skew):
    """group of every signer: even, or one group of n / 2 signers and the rest over d - 1 groups; every group occurs; scattered"""
    if skew and d > 1:
        g = np.concatenate([np.zeros(n // 2, dtype=np.int64), 1 + np.arange(n - n // 2, dtype=np.int64) % (d - 1)])
    else:
        g = np.arange(n, dtype=np.int64) % d
    return rng.permutation(g)


def measure(lib, cid, n, d, skew, sks, t_keys, steps, warmup):
    fp = 32 if cid == 0 else 48
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(17 * n + d + (5 if skew else 0) + cid)
    group = assignment(rng, n, d, skew)
    distinct = rng.integers(0, 256, size=(d, MSG), dtype=np.uint8)
    distinct[:, :4] = np.arange(d, dtype=">u4").view(np.uint8).reshape(d, 4)      # distinct by construction
    ssum = np.zeros(d, dtype=np.int64)
    np.add.at(ssum, group, sks)                              # below 2^51: exact, and below the group order
    gsigs = (ctypes.c_uint8 * (d * 2 * fp))()
    check(lib.bgls_sign_batch(cid, as_buf(be32(ssum)), as_buf(distinct), offs(d, MSG), d, gsigs), "sign_batch")
    agg = (ctypes.c_uint8 * (2 * fp))()
    check(lib.bgls_aggregate_points(cid, 1, gsigs, d, agg), "aggregate_points")
    t_sig = torch.frombuffer(bytearray(bytes(agg)), dtype=torch.uint8).to(dev)
    t_msgs = torch.from_numpy(np.ascontiguousarray(distinct[group])).to(dev)
    t_part = torch.zeros(12 * fp, dtype=torch.uint8, device=dev)
    t_flags = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def grouped_call():
        nd = ctypes.c_size_t(0)
        rc = check(lib.bgls_verify_aggregate_grouped_dev(cid, t_sig.data_ptr(), t_keys.data_ptr(), t_msgs.data_ptr(), MSG, MSG, n, ctypes.byref(nd), None, None),
                   "verify_aggregate_grouped_dev")
        if rc != 1 or nd.value != d:
            raise RuntimeError("grouped: verdict %d, %d groups of %d" % (rc, nd.value, d))

    def baseline_call():
        t_flags.zero_()
        torch.cuda.synchronize()
        check(lib.bgls_miller_product_dev(cid, t_sig.data_ptr(), t_keys.data_ptr(), t_msgs.data_ptr(), MSG, MSG, n, 0, t_part.data_ptr(), t_flags.data_ptr(), None),
              "miller_product_dev")
        rc = check(lib.bgls_final_verify_dev(cid, t_part.data_ptr(), 1, t_flags.data_ptr(), None), "final_verify_dev")
        if rc != 1:
            raise RuntimeError("baseline: verdict %d" % rc)

    res = {"curve": "altbn128" if cid == 0 else "bls12", "n": n, "d": d, "shape": "skew" if skew else "even", "largest_group": int(np.bincount(group).max())}
    all_ts, all_stages = timed(lib, (grouped_call, baseline_call), steps, warmup)
    for name, ts, stages in zip(("grouped", "baseline"), all_ts, all_stages):
        res[name] = {"s_median": round(statistics.median(ts), 6), "s_min": round(min(ts), 6), "stage_ms": stages}
    res["baseline_over_grouped"] = round(res["baseline"]["s_median"] / res["grouped"]["s_median"], 3)
    del t_msgs
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--logn", default="16,20")
    ap.add_argument("--shapes", default="even,skew")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        for lg in a.logn.split(","):
            cid, n = int(c), 1 << int(lg)
            sks, t_keys = signers(lib, cid, n, 4000 + cid)
            plan = []
            if "even" in a.shapes:
                plan += [(d, False) for d in (1, 64, n // 16, n // 4, n // 2, n)]
            if "skew" in a.shapes:
                plan += [(d, True) for d in (64, n // 4)]
            for d, skew in plan:
                recs.append(measure(lib, cid, n, d, skew, sks, t_keys, a.steps, a.warmup))
                print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            del t_keys
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "gpu_grouped", "results": recs}))


if __name__ == "__main__":
    main()
