#!/usr/bin/env python3
"""Cost of the distinct-message check against a prepared key set, from host buffers, with the hash inputs built on the device or on the host.

One instance per curve: --log2n signers (default 2^20), one 32-byte payload each, the keys resident as a key set uploaded with
BGLS_KEYS_PREPARE, a valid aggregate signature.  Two ways to verify it, timed alternately --reps times each (host clock around calls that
end in a device synchronise):
  (a) the older way: the caller puts every key's wire bytes in front of its payload (one numpy concatenation of the two row arrays, C
      speed, inside the timed window because every call has to do it) and calls bgls_verify_aggregate_h with allow_duplicates = 1;
  (b) bgls_verify_aggregate_distinct_h on the bare payloads.
Both verdicts are checked on every call.  Then (b) runs --reps more times with the stage timers on, for the key_msgs, h2c and miller
stage times (a run of its own: the timers add events to the stream).  Prints one JSON line: median, minimum and maximum of both ways,
the spread of (a) (maximum - minimum and standard deviation), bytes uploaded per call by either way, and the stage times of (b).
usage: python tools/gpu_distinct.py [--curves 0,1] [--log2n 20] [--reps 10] [--warmup 2]"""
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
import torch  # noqa: E402,F401  (one HIP runtime per process: see bgls_amd/_lib.py)

from bgls_amd import _lib  # noqa: E402

MSG = 32
KEYS_CHECK, KEYS_PREPARE = 1, 2
STAGES = ("key_msgs", "h2c", "miller")
u8p = ctypes.POINTER(ctypes.c_uint8)
u64p = ctypes.POINTER(ctypes.c_uint64)


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %d %s" % (what, rc, _lib.last_error()))
    return rc


def ptr(a, t=u8p):
    return a.ctypes.data_as(t)


def measure(lib, cid, n, reps, warmup):
    fp = 32 if cid == 0 else 48
    g1b, g2b = 2 * fp, 4 * fp
    rng = np.random.default_rng(2026 + cid)
    sks = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sks[:, 0] &= 0x0f                                     # below 2^252, hence below either group order
    sks[:, 31] |= 1                                       # never zero
    msgs = rng.integers(0, 256, size=(n, MSG), dtype=np.uint8)
    keys = np.empty((n, g2b), dtype=np.uint8)
    check(lib.bgls_scale_generator(cid, 2, ptr(sks), n, ptr(keys)), "scale_generator")
    off = np.arange(n + 1, dtype=np.uint64) * MSG
    off_pre = np.arange(n + 1, dtype=np.uint64) * (g2b + MSG)
    pre = np.concatenate([keys, msgs], axis=1)
    sigs = np.empty((n, g1b), dtype=np.uint8)
    check(lib.bgls_sign_batch(cid, ptr(sks), ptr(pre), ptr(off_pre, u64p), n, ptr(sigs)), "sign_batch")
    agg = np.empty(g1b, dtype=np.uint8)
    check(lib.bgls_aggregate_points(cid, 1, ptr(sigs), n, ptr(agg)), "aggregate_points")
    del sigs, pre
    h = ctypes.c_uint64()
    check(lib.bgls_keys_upload(cid, ptr(keys), n, None, 1, KEYS_PREPARE, ctypes.byref(h)), "keys_upload")

    def way_a():
        t0 = time.perf_counter()
        blob = np.concatenate([keys, msgs], axis=1)
        rc = lib.bgls_verify_aggregate_h(h, ptr(agg), ptr(blob), ptr(off_pre, u64p), n, 1)
        dt = time.perf_counter() - t0
        if rc != 1:
            raise RuntimeError("host-prefixed verification: %d %s" % (rc, _lib.last_error()))
        return dt

    def way_b():
        t0 = time.perf_counter()
        rc = lib.bgls_verify_aggregate_distinct_h(h, ptr(agg), ptr(msgs), ptr(off, u64p), n, None)
        dt = time.perf_counter() - t0
        if rc != 1:
            raise RuntimeError("device-prefixed verification: %d %s" % (rc, _lib.last_error()))
        return dt

    try:
        for _ in range(warmup):
            way_a()
            way_b()
        ta, tb = [], []
        for _ in range(reps):
            ta.append(way_a())
            tb.append(way_b())
        lib.bgls_profile_enable(1)
        for _ in range(reps):
            way_b()
        stage_ms = {}
        for s in STAGES:
            ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
            check(lib.bgls_profile_get(s.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "profile_get")
            stage_ms[s] = round(ms.value / reps, 4)
        lib.bgls_profile_enable(0)
    finally:
        lib.bgls_keys_free(h)

    def ms(ts):
        return {"median": round(1e3 * statistics.median(ts), 3), "min": round(1e3 * min(ts), 3), "max": round(1e3 * max(ts), 3)}

    return {"curve": "altbn128" if cid == 0 else "bls12", "signers": n, "payload_bytes": MSG, "reps": reps,
            "host_prefix_ms": ms(ta), "device_prefix_ms": ms(tb),
            "host_prefix_spread_ms": {"max_minus_min": round(1e3 * (max(ta) - min(ta)), 3), "stdev": round(1e3 * statistics.pstdev(ta), 3)},
            "device_over_host_median": round(statistics.median(tb) / statistics.median(ta), 4),
            "uploaded_bytes_host_prefix": n * (g2b + MSG) + 8 * (n + 1), "uploaded_bytes_device_prefix": n * MSG,
            "device_prefix_stage_ms": stage_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 2:
        raise SystemExit("--reps must be at least 2: the spread of the older way is part of the result")
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        recs.append(measure(lib, int(c), 1 << a.log2n, a.reps, a.warmup))
        print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "gpu_distinct", "results": recs}))


if __name__ == "__main__":
    main()
