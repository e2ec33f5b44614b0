#!/usr/bin/env python3
"""Throughput of bgls_ams_verify_batch_dev (n AmsVerifySignature calls, one verdict each) against a loop of the single path
(bgls.AmsVerifySignature: k + 1 hashing calls, a point sum and a three-pairing product per item) over the first --single-cap items of the
same shape, with the batch's inputs resident on the device.

Shapes (items x signers per item): 2^10 and 2^16 items at 4 and 64 signers.  One group key apk = a g2; index i is held by key i mod 8;
item b's signers are the window (b mod 64) .. (b mod 64) + k - 1 of the indices, its message is its own, and its signature is
(sum sk) H(0x00 || m_b) + a sum_i H(0x01 || apk || itoa(i)).  Every verdict is checked.  Also times the Miller stage of
bgls_verify_multi_sets_dev over as many one-key sets: twice that stage is what k_miller_ams replaces.  Prints one JSON line: us per
item of both ways and the per-call stage times.
usage: python tools/gpu_ams_batch.py [--curves 0,1] [--shapes 10x4,10x64,16x4,16x64] [--steps 3] [--warmup 1] [--single-cap 256]"""
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
NK = 8
WINDOWS = 64
STAGES = ("ams_msgs", "h2c", "sum_points", "miller", "epilogue", "final_exp")


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


def dev(data):
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).to(torch.device("cuda:0"))


def measure(lib, cid, ns, k, steps, warmup, cap):
    fp = 32 if cid == 0 else 48
    g1b, g2b = 2 * fp, 4 * fp
    r = ORDER[cid]
    rnd = random.Random(4000 + cid)
    sks = [rnd.randrange(1, r) for _ in range(NK)]
    a = rnd.randrange(1, r)
    pks, apk = (ctypes.c_uint8 * (NK * g2b))(), (ctypes.c_uint8 * g2b)()
    check(lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), NK, pks), "scale_generator")
    check(lib.bgls_scale_generator(cid, 2, B(a.to_bytes(32, "big")), 1, apk), "scale_generator")
    pks, apk = bytes(pks), bytes(apk)
    # a H2(apk, i) for every index in use, then per window its sum, the signers' key sum and secret sum
    n_idx = WINDOWS + k
    h2 = [b"\x01" + apk + str(i).encode() for i in range(n_idx)]
    mk = (ctypes.c_uint8 * (n_idx * g1b))()
    check(lib.bgls_sign_batch(cid, B(a.to_bytes(32, "big") * n_idx), B(b"".join(h2)), offs([len(m) for m in h2]), n_idx, mk), "sign_batch")
    mk = bytes(mk)
    wsum, wkey = (ctypes.c_uint8 * (WINDOWS * g1b))(), (ctypes.c_uint8 * (WINDOWS * g2b))()
    check(lib.bgls_aggregate_sets(cid, 1, B(b"".join(mk[w * g1b:(w + k) * g1b] for w in range(WINDOWS))), offs([k] * WINDOWS), WINDOWS, wsum), "aggregate_sets")
    check(lib.bgls_aggregate_sets(cid, 2, B(b"".join(pks[(i % NK) * g2b:(i % NK + 1) * g2b] for w in range(WINDOWS) for i in range(w, w + k))),
                                  offs([k] * WINDOWS), WINDOWS, wkey), "aggregate_sets")
    wsum, wkey = bytes(wsum), bytes(wkey)
    wsk = [sum(sks[i % NK] for i in range(w, w + k)) % r for w in range(WINDOWS)]
    msgs = rnd.randbytes(MSG * ns)
    h0 = b"".join(b"\x00" + msgs[b * MSG:(b + 1) * MSG] for b in range(ns))
    part = (ctypes.c_uint8 * (ns * g1b))()
    check(lib.bgls_sign_batch(cid, B(b"".join(wsk[b % WINDOWS].to_bytes(32, "big") for b in range(ns))), B(h0), offs([MSG + 1] * ns), ns, part), "sign_batch")
    part = bytes(part)
    sigs = (ctypes.c_uint8 * (ns * g1b))()
    check(lib.bgls_aggregate_sets(cid, 1, B(b"".join(part[b * g1b:(b + 1) * g1b] + wsum[(b % WINDOWS) * g1b:(b % WINDOWS + 1) * g1b] for b in range(ns))),
                                  offs([2] * ns), ns, sigs), "aggregate_sets")
    sigs = bytes(sigs)
    keys = b"".join(wkey[(b % WINDOWS) * g2b:(b % WINDOWS + 1) * g2b] for b in range(ns))
    t_apks, t_keys, t_sigs, t_msgs = dev(apk * ns), dev(keys), dev(sigs), dev(msgs)
    t_idx = ((torch.arange(ns, device=t_apks.device).view(ns, 1) % WINDOWS) + torch.arange(k, device=t_apks.device).view(1, k)).to(torch.int32).contiguous()
    t_soff = torch.arange(ns + 1, dtype=torch.int64, device=t_apks.device) * k
    t_one = torch.arange(ns + 1, dtype=torch.int64, device=t_apks.device)
    torch.cuda.synchronize()

    def batch_call():
        v = (ctypes.c_uint8 * ns)()
        rc = check(lib.bgls_ams_verify_batch_dev(cid, t_apks.data_ptr(), t_keys.data_ptr(), t_sigs.data_ptr(), t_idx.data_ptr(), t_soff.data_ptr(), ns, k,
                                                 t_msgs.data_ptr(), MSG, MSG, v, None, None), "ams_verify_batch_dev")
        if rc != ns or sum(v) != ns:
            raise RuntimeError("batch: %d of %d accepted" % (rc, ns))

    def sets_call():                        # ns one-key sets through k_miller_sets: timing only, the verdicts are 0
        v = (ctypes.c_uint8 * ns)()
        check(lib.bgls_verify_multi_sets_dev(cid, t_sigs.data_ptr(), t_keys.data_ptr(), t_one.data_ptr(), ns, 1, t_msgs.data_ptr(), MSG, MSG, v, None, None),
              "verify_multi_sets_dev")

    res = {"curve": "altbn128" if cid == 0 else "bls12", "items": ns, "signers_per_item": k}
    for _ in range(warmup):
        batch_call()
    times = []
    lib.bgls_profile_enable(1)
    for _ in range(steps):
        t0 = time.perf_counter()
        batch_call()
        times.append(time.perf_counter() - t0)
    res["stage_ms"] = stage_times(lib, steps)
    lib.bgls_profile_enable(0)
    dt = sum(times) / steps
    res["batch_ms_per_call"] = round(1e3 * dt, 3)
    res["batch_ms_min_max"] = [round(1e3 * min(times), 3), round(1e3 * max(times), 3)]
    res["batch_us_per_item"] = round(1e6 * dt / ns, 3)
    res["stage_us_per_item"] = {s: round(1e3 * ms / ns, 4) for s, ms in res["stage_ms"].items()}
    sets_call()
    per_call = []
    for _ in range(steps):
        lib.bgls_profile_enable(1)
        sets_call()
        per_call.append(stage_times(lib, 1).get("miller", 0))
        lib.bgls_profile_enable(0)
    res["sets_miller_ms"] = per_call
    res["miller_vs_two_sets"] = round(res["stage_ms"].get("miller", 0) / (2 * sum(per_call) / steps), 3) if sum(per_call) else None
    m1 = min(ns, cap)
    if m1:
        from bgls_amd import Altbn128, Bls12, bgls
        from bgls_amd.curves import Point, G1, G2
        cv = Altbn128 if cid == 0 else Bls12
        p_apk = Point(cv, G2, apk)

        def single_loop():
            for b in range(m1):
                w = b % WINDOWS
                if not bgls.AmsVerifySignature(cv, p_apk, list(range(w, w + k)), Point(cv, G2, keys[b * g2b:(b + 1) * g2b]),
                                               Point(cv, G1, sigs[b * g1b:(b + 1) * g1b]), msgs[b * MSG:(b + 1) * MSG]):
                    raise RuntimeError("single: item %d refused" % b)
        single_loop()
        t0 = time.perf_counter()
        single_loop()
        res["single_us_per_item"] = round(1e6 * (time.perf_counter() - t0) / m1, 2)
        res["single_items_timed"] = m1
        res["batch_vs_single"] = round(res["single_us_per_item"] / res["batch_us_per_item"], 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--shapes", default="10x4,10x64,16x4,16x64")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--single-cap", type=int, default=256)
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        for sh in a.shapes.split(","):
            l2, k = sh.split("x")
            recs.append(measure(lib, int(c), 1 << int(l2), int(k), a.steps, a.warmup, a.single_cap))
            print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
    print(json.dumps({"tool": "gpu_ams_batch", "results": recs}))


if __name__ == "__main__":
    main()
