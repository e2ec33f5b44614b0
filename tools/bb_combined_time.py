#!/usr/bin/env python3
"""bgls_bb_verify_batch_combined_dev against bgls_bb_verify_batch_dev on the same valid items, inputs resident on the device, one call in
flight, both calls in the same process and alternating repetition by repetition:

  per_item   bgls_bb_verify_batch_dev: one verdict per item, one Miller accumulator and one final exponentiation per item
  one_group  bgls_bb_verify_batch_combined_dev with group_off = NULL: one verdict for the batch
  groups     the same with groups of --group items (64: what VerifyBatchLocated asks for)

A repetition is a host clock around one call (each call ends in a stream synchronise).  Prints one JSON line per curve and n: the
median, the smallest and the largest repetition of each form in ms, and the per-stage split of the two combined forms in ms per call
(bgls_profile_*).  Every verdict is checked (all items valid).
usage: python tools/bb_combined_time.py [--curves 0,1] [--logn 12,16] [--reps 7] [--warmup 2] [--group 64]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from bgls_amd import _lib  # noqa: E402
from gpu_bb_verify import check, items  # noqa: E402

STAGES = ("bb_keys", "rlc", "scatter", "miller", "reduce", "epilogue", "final_exp")


def stage_split(lib):
    res = {}
    for s in STAGES:
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        check(lib.bgls_profile_get(s.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "profile_get")
        if cnt.value:
            res[s] = round(ms.value, 3)
    return res


def measure(lib, cid, logns, reps, warmup, group):
    dev = torch.device("cuda:0")
    nmax = 1 << max(logns)
    sig, rs, keys, ms, _ = items(lib, cid, nmax, 3000 + cid)
    d = [torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev) for b in (sig, rs, keys, ms)]
    ptr = [t.data_ptr() for t in d]
    seed = (ctypes.c_uint8 * 32)(*os.urandom(32))
    torch.cuda.synchronize()
    for logn in logns:
        n = 1 << logn
        cuts = list(range(0, n, group)) + [n]
        goff = (ctypes.c_uint64 * len(cuts))(*cuts)
        v = (ctypes.c_uint8 * n)()

        def per_item():
            assert check(lib.bgls_bb_verify_batch_dev(cid, *ptr, n, v, None, None), "bb_verify_batch_dev") == n

        def one_group():
            assert check(lib.bgls_bb_verify_batch_combined_dev(cid, *ptr, n, None, 1, seed, v, None, None), "bb_verify_batch_combined_dev") == 1

        def groups():
            assert check(lib.bgls_bb_verify_batch_combined_dev(cid, *ptr, n, goff, len(cuts) - 1, seed, v, None, None),
                         "bb_verify_batch_combined_dev") == len(cuts) - 1

        forms = {"per_item": per_item, "one_group": one_group, "groups": groups}
        times = {k: [] for k in forms}
        for rep in range(warmup + reps):
            for k, fn in forms.items():                      # alternating: a drift of the machine falls on every form alike
                t0 = time.perf_counter()
                fn()
                if rep >= warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3)
        row = {"curve": ["altbn128", "bls12"][cid], "n": n, "group": group, "reps": reps}
        for k, ts in times.items():
            row[k + "_ms"] = {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}
        for k in ("one_group", "groups"):
            check(lib.bgls_profile_enable(1), "profile_enable")
            forms[k]()
            row[k + "_stage_ms"] = stage_split(lib)
            check(lib.bgls_profile_enable(0), "profile_enable")
        print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--logn", default="12,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--group", type=int, default=64)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    for cid in [int(c) for c in a.curves.split(",")]:
        measure(lib, cid, [int(x) for x in a.logn.split(",")], a.reps, a.warmup, a.group)


if __name__ == "__main__":
    main()
