#!/usr/bin/env python3
"""Time of bgls_verify_aggregate_grouped_keys_dev (grouped aggregate verification whose keys are the sub-slice of a resident key set that a
signer bitmap selects) against the ways such an instance could be verified before it, on the same machine in the same session, inputs
resident on the device:

  new  one bgls_verify_aggregate_grouped_keys_dev call per step (bitmap NULL at 100 % participation, a random 50 % bitmap otherwise)
  A    bgls_miller_product_keys_dev(check_duplicates = 0) + bgls_final_verify_dev on the same key set (100 % rows only): n hashes, n + 1 loops
  B    bgls_verify_aggregate_grouped_dev on the selected keys' wire bytes already gathered in HBM (gather and upload not charged)
  C    d = n only: bgls_miller_product_dev(check_duplicates = 0) + bgls_final_verify_dev on those gathered keys: B's own ungrouped baseline

n registered keys, k selected, d distinct 32-byte messages dealt over the selected keys (even: spread evenly; skew: one message for k / 2
signers, the rest over d - 1).  Secret keys are below 2^31, so a group's secret sum is an exact integer; the aggregate signature is the sum
of the d group signatures.  Every verdict and n_groups is checked.  The ways alternate step by step.  With --sweep the new call is also
timed under bgls_set_group_small 0 / 8 / 32 / 128 at d = n, n / 4, n / 16 (100 %).  Prints one JSON line; every record also goes to stderr.
usage: python tools/gpu_grouped_keys.py [--curves 0,1] [--logn 16,20] [--steps 5] [--warmup 1] [--shapes even,skew] [--sweep [--sweep-divs 1,4,16]]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bgls_amd import _lib  # noqa: E402
import gpu_grouped as gg  # noqa: E402

MSG = gg.MSG
check, as_buf, offs, be32 = gg.check, gg.as_buf, gg.offs, gg.be32
SMALLS = (0, 8, 32, 128)


def key_set(lib, cid, n, seed):
    fp = 32 if cid == 0 else 48
    rng = np.random.default_rng(seed)
    sks = rng.integers(1, 1 << 31, size=n, dtype=np.int64)
    keys = (ctypes.c_uint8 * (n * 4 * fp))()
    check(lib.bgls_scale_generator(cid, 2, as_buf(be32(sks)), n, keys), "scale_generator")
    h = ctypes.c_uint64()
    check(lib.bgls_keys_upload(cid, keys, n, (ctypes.c_int * 1)(0), 1, 0, ctypes.byref(h)), "keys_upload")
    t_keys = torch.frombuffer(bytearray(bytes(keys)), dtype=torch.uint8).to(torch.device("cuda:0")).view(n, 4 * fp)
    return sks, t_keys, h.value


def spread(ts):
    return max(ts) - min(ts)


def measure(lib, cid, n, h, sks, t_keys, d_of, skew, half, steps, warmup, smalls=None):
    fp = 32 if cid == 0 else 48
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(19 * n + (7 if half else 0) + (5 if skew else 0) + cid)
    sel = np.flatnonzero(rng.integers(0, 2, size=n)) if half else np.arange(n)
    k = int(sel.size)
    d = max(1, d_of(k))
    group = gg.assignment(rng, k, d, skew)
    distinct = rng.integers(0, 256, size=(d, MSG), dtype=np.uint8)
    distinct[:, :4] = np.arange(d, dtype=">u4").view(np.uint8).reshape(d, 4)
    ssum = np.zeros(d, dtype=np.int64)
    np.add.at(ssum, group, sks[sel])
    gsigs = (ctypes.c_uint8 * (d * 2 * fp))()
    check(lib.bgls_sign_batch(cid, as_buf(be32(ssum)), as_buf(distinct), offs(d, MSG), d, gsigs), "sign_batch")
    agg = (ctypes.c_uint8 * (2 * fp))()
    check(lib.bgls_aggregate_points(cid, 1, gsigs, d, agg), "aggregate_points")
    t_sig = torch.frombuffer(bytearray(bytes(agg)), dtype=torch.uint8).to(dev)
    t_msgs = torch.from_numpy(np.ascontiguousarray(distinct[group])).to(dev)
    words = np.zeros((n + 31) // 32, dtype=np.uint32)
    np.bitwise_or.at(words, sel >> 5, (np.uint32(1) << (sel & 31).astype(np.uint32)))
    t_map = torch.from_numpy(words.view(np.uint8).copy()).to(dev) if half else None
    t_gath = t_keys if not half else t_keys[torch.from_numpy(sel).to(dev)].contiguous()
    t_part = torch.zeros(12 * fp, dtype=torch.uint8, device=dev)
    t_flags = torch.zeros(4, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def new_call():
        nd = ctypes.c_size_t(0)
        rc = check(lib.bgls_verify_aggregate_grouped_keys_dev(h, t_sig.data_ptr(), t_map.data_ptr() if half else None, t_map.numel() if half else 0, t_msgs.data_ptr(),
                                                              MSG, MSG, k, ctypes.byref(nd), None, None), "verify_aggregate_grouped_keys_dev")
        if rc != 1 or nd.value != d:
            raise RuntimeError("new: verdict %d, %d groups of %d" % (rc, nd.value, d))

    def b_call():
        nd = ctypes.c_size_t(0)
        rc = check(lib.bgls_verify_aggregate_grouped_dev(cid, t_sig.data_ptr(), t_gath.data_ptr(), t_msgs.data_ptr(), MSG, MSG, k, ctypes.byref(nd), None, None),
                   "verify_aggregate_grouped_dev")
        if rc != 1 or nd.value != d:
            raise RuntimeError("B: verdict %d, %d groups of %d" % (rc, nd.value, d))

    def final():
        rc = check(lib.bgls_final_verify_dev(cid, t_part.data_ptr(), 1, t_flags.data_ptr(), None), "final_verify_dev")
        if rc != 1:
            raise RuntimeError("baseline: verdict %d" % rc)

    def a_call():
        t_flags.zero_()
        torch.cuda.synchronize()
        check(lib.bgls_miller_product_keys_dev(h, t_sig.data_ptr(), t_msgs.data_ptr(), MSG, MSG, n, 0, t_part.data_ptr(), t_flags.data_ptr(), None), "miller_product_keys_dev")
        final()

    def c_call():
        t_flags.zero_()
        torch.cuda.synchronize()
        check(lib.bgls_miller_product_dev(cid, t_sig.data_ptr(), t_gath.data_ptr(), t_msgs.data_ptr(), MSG, MSG, k, 0, t_part.data_ptr(), t_flags.data_ptr(), None),
              "miller_product_dev")
        final()

    res = {"curve": "altbn128" if cid == 0 else "bls12", "n": n, "selected": k, "d": d, "shape": "skew" if skew else "even", "participation": 50 if half else 100}
    if smalls is not None:
        res["sweep"] = {}
        try:
            for s in smalls:
                check(lib.bgls_set_group_small(s), "set_group_small")
                ts, stages = gg.timed(lib, (new_call,), steps, warmup)
                res["sweep"][str(s)] = {"ms_median": round(1e3 * statistics.median(ts[0]), 4), "ms_min": round(1e3 * min(ts[0]), 4), "ms_max": round(1e3 * max(ts[0]), 4),
                                        "stage_ms": stages[0]}
        finally:
            lib.bgls_set_group_small(32)
        return res
    ways = [("new", new_call), ("B", b_call)]
    if not half:
        ways.append(("A", a_call))
    if d == k:
        ways.append(("C", c_call))
    all_ts, all_stages = gg.timed(lib, tuple(fn for _, fn in ways), steps, warmup)
    for (name, _), ts, stages in zip(ways, all_ts, all_stages):
        res[name] = {"ms_median": round(1e3 * statistics.median(ts), 4), "ms_min": round(1e3 * min(ts), 4), "ms_max": round(1e3 * max(ts), 4), "stage_ms": stages}
    res["new_minus_B_ms"] = round(res["new"]["ms_median"] - res["B"]["ms_median"], 4)
    res["allowed_ms"] = round(1e3 * max(spread(all_ts[0]), spread(all_ts[1])), 4)
    res["within"] = res["new_minus_B_ms"] <= res["allowed_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--logn", default="16,20")
    ap.add_argument("--shapes", default="even,skew")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-divs", default="1,4,16", help="with --sweep: d = n / div for every div")
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    for c in a.curves.split(","):
        for lg in a.logn.split(","):
            cid, n = int(c), 1 << int(lg)
            sks, t_keys, h = key_set(lib, cid, n, 5000 + cid)
            plan = []
            if a.sweep:
                plan = [(int(div), False, False, SMALLS) for div in a.sweep_divs.split(",")]
            else:
                for half in (False, True):
                    if "even" in a.shapes:
                        plan += [(0, False, half, None), (-64, False, half, None)] + [(div, False, half, None) for div in (16, 4, 2, 1)]
                    if "skew" in a.shapes:
                        plan += [(-64, True, half, None), (4, True, half, None)]
            for div, skew, half, smalls in plan:
                d_of = (lambda k: 1) if div == 0 else (lambda k, v=-div: min(v, k)) if div < 0 else (lambda k, v=div: k // v)
                recs.append(measure(lib, cid, n, h, sks, t_keys, d_of, skew, half, a.steps, a.warmup, smalls))
                print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
            check(lib.bgls_keys_free(h), "keys_free")
            del t_keys
            torch.cuda.empty_cache()
    print(json.dumps({"tool": "gpu_grouped_keys", "sweep": bool(a.sweep), "results": recs}))


if __name__ == "__main__":
    main()
