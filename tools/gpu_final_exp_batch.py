#!/usr/bin/env python3
"""Per-item time of the throughput final exponentiation (bgls_final_exp_batch_dev: k_finalxt_batch, ten items per wave) against the
latency kernel launched once per item (k_finalx_batch, the tail of every per-item-verdict batch), in ONE run, alternating the two:

  new   bgls_final_exp_batch_dev on n resident GT-size values, both outputs on the device; host clock around calls that synchronise
  old   the final_exp stage (bgls_profile_get, device events) of bgls_bb_verify_batch_dev over n items, whose tail is k_finalx_batch
        over n + 1 values (the items and the reference pair); divided by n + 1

Inputs of `new` are the GT elements the `old` call hands back for the same items (gt_out): the same batch one exponentiation further.
Both chains are fixed by the public exponent, so the time does not depend on the values; the Miller partials themselves stay inside the
Boneh-Boyen call.  The outputs of `new` are checked against k_finalx_batch on the same inputs through bgls_final_verify_dev item by item
for a sample, and its is_one marks against the bytes.  Each figure is the median of --reps alternated rounds; the spread (min .. max)
is printed beside it.  One JSON line per curve.
usage: python tools/gpu_final_exp_batch.py [--curves 0,1] [--logn 12,16] [--reps 5]"""
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


def stage_ms(lib, name):
    ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
    check(lib.bgls_profile_get(name.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "profile_get")
    return ms.value, cnt.value


def measure(lib, cid, logns, reps):
    fp = 32 if cid == 0 else 48
    gtb = 12 * fp
    dev = torch.device("cuda:0")
    out = {"curve": ["altbn128", "bls12"][cid]}
    nmax = 1 << max(logns)
    sig, rs, keys, ms, _ = items(lib, cid, nmax, 3000 + cid)
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)    # noqa: E731
    d_sig, d_rs, d_keys, d_ms = to_dev(sig), to_dev(rs), to_dev(keys), to_dev(ms)
    torch.cuda.synchronize()
    for logn in logns:
        n = 1 << logn
        v = (ctypes.c_uint8 * n)()
        gt = (ctypes.c_uint8 * (n * gtb))()

        def old(with_gt=False):
            assert check(lib.bgls_bb_verify_batch_dev(cid, d_sig.data_ptr(), d_rs.data_ptr(), d_keys.data_ptr(), d_ms.data_ptr(), n, v,
                                                      gt if with_gt else None, None), "bb_verify_batch_dev") == n

        old(True)
        d_in = to_dev(bytes(gt))
        d_out = torch.zeros(n * gtb, dtype=torch.uint8, device=dev)
        d_one = torch.zeros(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

        def new():
            check(lib.bgls_final_exp_batch_dev(cid, d_in.data_ptr(), n, d_out.data_ptr(), d_one.data_ptr(), None), "final_exp_batch_dev")

        # results first: a sample of items against the latency kernel (bgls_final_verify_dev: k_finalx on ONE value, verdict = "is one")
        new()
        ones = d_one.cpu().numpy()
        res = bytes(d_out.cpu().numpy())
        one = bytes(gtb - 1) + b"\x01"
        for b in range(0, n, max(1, n // 64)):
            assert ones[b] == (1 if res[b * gtb:(b + 1) * gtb] == one else 0), b
            assert check(lib.bgls_final_verify_dev(cid, d_in.data_ptr() + b * gtb, 1, None, None), "final_verify_dev") == int(ones[b]), b
        old()
        t_new, t_old = [], []
        for _ in range(reps):                                  # alternate the two
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            new()                                              # synchronises its stream before it returns
            t_new.append((time.perf_counter() - t0) / n * 1e6)
            check(lib.bgls_profile_enable(1), "profile_enable")
            old()
            ms_f, cnt = stage_ms(lib, "final_exp")
            check(lib.bgls_profile_enable(0), "profile_enable")
            assert cnt == 1
            t_old.append(ms_f / (n + 1) * 1e3)
        # the new call's own final_exp stage by device events, for a like-for-like figure beside the host clock
        check(lib.bgls_profile_enable(1), "profile_enable")
        new()
        ms_n, cnt = stage_ms(lib, "final_exp")
        check(lib.bgls_profile_enable(0), "profile_enable")
        assert cnt == 1
        f = lambda xs: {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}    # noqa: E731
        out["n=2^%d" % logn] = {"new_call_us_per_item": f(t_new), "new_stage_us_per_item": round(ms_n / n * 1e3, 4), "old_stage_us_per_item": f(t_old),
                                "speedup_stage_over_stage": round(statistics.median(t_old) / (ms_n / n * 1e3), 2)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--logn", default="12,16")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    for cid in [int(c) for c in a.curves.split(",")]:
        print(json.dumps(measure(lib, cid, [int(x) for x in a.logn.split(",")], a.reps)), flush=True)


if __name__ == "__main__":
    main()
