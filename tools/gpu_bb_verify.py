#!/usr/bin/env python3
"""Throughput of bgls_bb_verify_batch_dev (n independent Boneh-Boyen verifications, bbsigs.Verify, one verdict each) with inputs
resident on the device, against two other ways of doing a single-pairing check per item:

  bb        one bgls_bb_verify_batch_dev call per step, n = 2^10, 2^16, 2^20
  stepwise  what a Go caller of bbsigs.Verify does today through the per-point calls: bgls_scale_generator (m g2), bgls_point_add (U),
            bgls_scale_points (r V), bgls_point_add, bgls_pair -- five C calls per item, timed over --stepwise-n items, per item
  sets      bgls_verify_multi_sets_dev with one-key sets at the same n (VerifySingleSignature: the closest existing one-pairing-per-item
            batch, which also hashes each message to G1)

Every verdict of `bb` and `sets` is checked (all items valid).  Prints one JSON line per curve: us per item of each way and the per-item
stage split of `bb` (bgls_profile_*: bb_keys, miller, epilogue, final_exp), one call in flight.
usage: python tools/gpu_bb_verify.py [--curves 0,1] [--logn 10,16,20] [--steps 3] [--warmup 1] [--stepwise-n 256]"""
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
STAGES = ("bb_keys", "miller", "epilogue", "final_exp", "h2c")


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %d %s" % (what, rc, _lib.last_error()))
    return rc


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")


def be(ks):
    return b"".join(k.to_bytes(32, "big") for k in ks)


def scale_gen(lib, cid, group, ks, size):
    o = (ctypes.c_uint8 * (len(ks) * size))()
    check(lib.bgls_scale_generator(cid, group, B(be(ks)), len(ks), o), "scale_generator")
    return bytes(o)


def items(lib, cid, n, seed):
    """n valid items: sigma (n G1), r, U || V (n x 2 G2), m, as bytes"""
    fp = 32 if cid == 0 else 48
    q = ORDER[cid]
    rnd = random.Random(seed)
    xs = [rnd.randrange(1, q) for _ in range(n)]
    ys = [rnd.randrange(1, q) for _ in range(n)]
    rs = [rnd.randrange(1, q) for _ in range(n)]
    ms = [rnd.randrange(0, q) for _ in range(n)]
    us, vs = scale_gen(lib, cid, 2, xs, 4 * fp), scale_gen(lib, cid, 2, ys, 4 * fp)
    sig = scale_gen(lib, cid, 1, [pow((x + m + y * r) % q, -1, q) for x, y, m, r in zip(xs, ys, ms, rs)], 2 * fp)
    g2b = 4 * fp
    keys = b"".join(us[i * g2b:(i + 1) * g2b] + vs[i * g2b:(i + 1) * g2b] for i in range(n))
    return sig, be(rs), keys, be(ms), us


def stage_split(lib, calls, n):
    res = {}
    for s in STAGES:
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        check(lib.bgls_profile_get(s.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "profile_get")
        if cnt.value:
            res[s] = round(ms.value / calls / n * 1e3, 4)             # us per item
    return res


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def measure(lib, cid, logns, steps, warmup, step_n):
    fp = 32 if cid == 0 else 48
    g1b, g2b, gtb = 2 * fp, 4 * fp, 12 * fp
    dev = torch.device("cuda:0")
    out = {"curve": ["altbn128", "bls12"][cid]}
    nmax = 1 << max(logns)
    sig, rs, keys, ms, us = items(lib, cid, nmax, 3000 + cid)
    to_dev = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)    # noqa: E731
    d_sig, d_rs, d_keys, d_ms, d_us = to_dev(sig), to_dev(rs), to_dev(keys), to_dev(ms), to_dev(us)
    # one-key sets: set b = key U_b, a signature of U_b's secret on a 32-byte message (the timing needs valid sets only)
    rnd = random.Random(4000 + cid)
    sks = [rnd.randrange(1, ORDER[cid]) for _ in range(nmax)]
    set_keys = scale_gen(lib, cid, 2, sks, g2b)
    msgs = rnd.randbytes(MSG * nmax)
    off = (ctypes.c_uint64 * (nmax + 1))(*range(0, MSG * (nmax + 1), MSG))
    set_sigs = (ctypes.c_uint8 * (nmax * g1b))()
    check(lib.bgls_sign_batch(cid, B(be(sks)), B(msgs), off, nmax, set_sigs), "sign_batch")
    d_ssig, d_skeys, d_msgs = to_dev(bytes(set_sigs)), to_dev(set_keys), to_dev(msgs)
    d_koff = torch.arange(nmax + 1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for logn in logns:
        n = 1 << logn
        v = (ctypes.c_uint8 * n)()

        def bb():
            assert check(lib.bgls_bb_verify_batch_dev(cid, d_sig.data_ptr(), d_rs.data_ptr(), d_keys.data_ptr(), d_ms.data_ptr(), n, v, None, None),
                         "bb_verify_batch_dev") == n

        def sets():
            assert check(lib.bgls_verify_multi_sets_dev(cid, d_ssig.data_ptr(), d_skeys.data_ptr(), d_koff.data_ptr(), n, 1, d_msgs.data_ptr(), MSG,
                                                        MSG, v, None, None), "verify_multi_sets_dev") == n

        t_bb = timed(bb, steps, warmup)
        check(lib.bgls_profile_enable(1), "profile_enable")
        bb()
        torch.cuda.synchronize()
        split = stage_split(lib, 1, n)
        check(lib.bgls_profile_enable(0), "profile_enable")
        t_sets = timed(sets, steps, warmup)
        out["n=2^%d" % logn] = {"bb_us_per_item": round(t_bb / n * 1e6, 4), "sets_us_per_item": round(t_sets / n * 1e6, 4),
                                "bb_items_per_s": round(n / t_bb), "bb_stage_us_per_item": split}
    # the stepwise per-point path, host buffers as a Go caller holds them
    gt = (ctypes.c_uint8 * gtb)()
    q, t, mg2, rv = [(ctypes.c_uint8 * g2b)() for _ in range(4)]
    zero = B(b"\0")

    def stepwise():
        for i in range(step_n):
            check(lib.bgls_scale_generator(cid, 2, B(ms[32 * i:32 * i + 32]), 1, mg2), "scale_generator")
            check(lib.bgls_point_add(cid, 2, mg2, B(keys[2 * g2b * i:2 * g2b * i + g2b]), t), "point_add")
            check(lib.bgls_scale_points(cid, 2, B(keys[2 * g2b * i + g2b:2 * g2b * (i + 1)]), B(rs[32 * i:32 * i + 32]), zero, 1, rv), "scale_points")
            check(lib.bgls_point_add(cid, 2, t, rv, q), "point_add")
            check(lib.bgls_pair(cid, B(sig[g1b * i:g1b * (i + 1)]), q, gt), "pair")

    out["stepwise_us_per_item"] = round(timed(stepwise, 1, 1) / step_n * 1e6, 2)
    out["stepwise_n"] = step_n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--logn", default="10,16,20")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--stepwise-n", type=int, default=256)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    for cid in [int(c) for c in a.curves.split(",")]:
        print(json.dumps(measure(lib, cid, [int(x) for x in a.logn.split(",")], a.steps, a.warmup, a.stepwise_n)), flush=True)


if __name__ == "__main__":
    main()
