#!/usr/bin/env python3
"""Key sets from compressed keys: bgls_keys_upload_compressed (one call: the compressed bytes up, the one-pass kernel k_wirex per shard)
against the route a caller had before it, on the same machine in the same process:

  old   bgls_decompress_points (n compressed keys up, n uncompressed keys and n ok bytes down), then bgls_keys_upload(BGLS_KEYS_CHECK)
        (the uncompressed keys up again, k_g2_parse with the subgroup test a second time), then bgls_keys_free
  new   bgls_keys_upload_compressed, then bgls_keys_free

Upload and free are inside the timed region of both; the ways alternate repetition by repetition; median, min and max.
Kernel-only device time per key, recorded beside it:
  k_wirex          hip events around bgls_decompress_points_dev over resident input (G2)
  k_decompress_*   the "sum_points" stage of bgls_decompress_points (hip events around the kernel, bgls_profile_*)
  k_g2_parse       no event brackets it: its subgroup test is taken as T(bgls_keys_upload with CHECK) - T(without), host clock, medians;
                   parse and curve check are not counted, so the old pair is UNDER-estimated by this column
Writes profiles/keys_compressed.json and prints the record.  The clock is not pinned or sampled: wall-clock and event times at the
machine's default power state (`clock`), and `counters_from` names this tool's run.
The first point of the process is measured once and thrown away (kept in the record as `discarded_first_point`), every point then gets
two warm-ups and --rounds runs of --steps repetitions; `s_all` keeps every repetition.  --markdown writes the rows of DESIGN.md's tables.
usage: python tools/gpu_keys_compressed.py [--curves 0,1] [--logn 16,20] [--steps 5] [--rounds 2] [--out profiles/keys_compressed.json] [--markdown rows.md]"""
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


def check(rc, what):
    if rc < 0:
        raise RuntimeError("%s failed: %d %s" % (what, rc, _lib.last_error()))
    return rc


def make_keys(lib, cid, n):
    fp = 32 if cid == 0 else 48
    rng = np.random.default_rng(5000 + cid)
    sks = rng.integers(1, 1 << 62, size=n, dtype=np.int64)
    raw = b"".join(int(s).to_bytes(32, "big") for s in sks)
    keys = (ctypes.c_uint8 * (n * 4 * fp))()
    check(lib.bgls_scale_generator(cid, 2, (ctypes.c_uint8 * len(raw)).from_buffer_copy(raw), n, keys), "scale_generator")
    comp = (ctypes.c_uint8 * (n * 2 * fp))()
    check(lib.bgls_compress_points(cid, 2, keys, n, comp), "compress_points")
    return keys, comp


def stats(ts):
    return {"s_median": round(statistics.median(ts), 6), "s_min": round(min(ts), 6), "s_max": round(max(ts), 6)}


def measure(lib, cid, logn, steps, rounds=2):
    fp, n = 32 if cid == 0 else 48, 1 << logn
    keys, comp = make_keys(lib, cid, n)
    devs = (ctypes.c_int * 1)(0)
    out, ok = (ctypes.c_uint8 * (n * 4 * fp))(), (ctypes.c_uint8 * n)()

    def upload(flags):
        h = ctypes.c_uint64()
        check(lib.bgls_keys_upload(cid, out if flags else keys, n, devs, 1, flags, ctypes.byref(h)), "keys_upload")
        check(lib.bgls_keys_free(h.value), "keys_free")

    def old():
        check(lib.bgls_decompress_points(cid, 2, comp, n, out, ok), "decompress_points")
        upload(1)

    def new():
        h, bad = ctypes.c_uint64(), ctypes.c_size_t()
        check(lib.bgls_keys_upload_compressed(cid, comp, n, devs, 1, 0, ctypes.byref(h), ctypes.byref(bad)), "keys_upload_compressed")
        check(lib.bgls_keys_free(h.value), "keys_free")

    def plain():
        upload(0)

    def checked():
        upload(1)

    fns = (old, new, plain, checked)
    for _ in range(2):                                   # two warm-ups: the second runs with every workspace at its final size
        for fn in fns:
            fn()
    if bytes(out) != bytes(keys) or bytes(ok) != b"\x01" * n:
        raise RuntimeError("decompression differs from the keys that were compressed")
    # `rounds` runs of `steps` alternating repetitions each: the spread of a way's medians from run to run is what the requirement names
    runs = [[[] for _ in fns] for _ in range(rounds)]
    for r in range(rounds):
        for _ in range(steps):
            for k, fn in enumerate(fns):
                t0 = time.perf_counter()
                fn()
                runs[r][k].append(time.perf_counter() - t0)
    ts = [sum((runs[r][k] for r in range(rounds)), []) for k in range(len(fns))]
    res = {"curve": "altbn128" if cid == 0 else "bls12", "keys": n, "old": stats(ts[0]), "new": stats(ts[1])}
    for name, k in (("old", 0), ("new", 1)):
        res[name]["s_all"] = [[round(t, 6) for t in runs[r][k]] for r in range(rounds)]
        res[name]["run_medians"] = [round(statistics.median(runs[r][k]), 6) for r in range(rounds)]
    res["old_vs_new"] = round(res["old"]["s_median"] / res["new"]["s_median"], 3)
    spread = max(res["old"]["s_max"] - res["old"]["s_min"], res["new"]["s_max"] - res["new"]["s_min"])
    res["spread_s"] = round(spread, 6)
    res["new_faster_by_more_than_spread"] = bool(res["old"]["s_median"] - res["new"]["s_median"] > spread)
    mspread = max(max(res[w]["run_medians"]) - min(res[w]["run_medians"]) for w in ("old", "new"))
    res["median_spread_s"] = round(mspread, 6)
    res["new_faster_by_more_than_median_spread"] = bool(min(res["old"]["run_medians"]) - max(res["new"]["run_medians"]) > mspread)
    res["every_new_below_every_old"] = bool(res["new"]["s_max"] < res["old"]["s_min"])
    # kernel-only
    t_in = torch.frombuffer(bytearray(bytes(comp)), dtype=torch.uint8).to("cuda:0")
    t_out = torch.empty(n * 4 * fp, dtype=torch.uint8, device="cuda:0")
    t_ok = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream()
    ev = []
    for k in range(steps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
        check(lib.bgls_decompress_points_dev(cid, 2, t_in.data_ptr(), n, t_out.data_ptr(), t_ok.data_ptr(), ctypes.c_void_p(st.cuda_stream)), "decompress_points_dev")
        b.record(st)
        torch.cuda.synchronize()
        if k:
            ev.append(a.elapsed_time(b))
    if int(t_ok.sum().item()) != n:
        raise RuntimeError("k_wirex refused a key")
    lib.bgls_profile_enable(1)
    for _ in range(steps):
        check(lib.bgls_decompress_points(cid, 2, comp, n, out, ok), "decompress_points")
    ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
    check(lib.bgls_profile_get(b"sum_points", ctypes.byref(ms), ctypes.byref(cnt)), "profile_get")
    lib.bgls_profile_enable(0)
    dec_ms = ms.value / max(1, cnt.value)
    sub_ms = (statistics.median(ts[3]) - statistics.median(ts[2])) * 1e3
    res["kernel_us_per_key"] = {"k_wirex": round(statistics.median(ev) * 1e3 / n, 4), "k_wirex_min_max_ms": [round(min(ev), 3), round(max(ev), 3)],
                                "k_decompress": round(dec_ms * 1e3 / n, 4), "k_g2_parse_subgroup_test_by_difference": round(sub_ms * 1e3 / n, 4)}
    res["kernel_us_per_key"]["old_pair"] = round(res["kernel_us_per_key"]["k_decompress"] + res["kernel_us_per_key"]["k_g2_parse_subgroup_test_by_difference"], 4)
    del t_in, t_out, t_ok
    torch.cuda.empty_cache()
    return res


def markdown(recs):
    """the rows of the DESIGN.md section: whole calls in ms, kernel-only in us per key"""
    ms = lambda v: "%.2f" % (v * 1e3)
    out = ["| curve, n | old (min-max) | new (min-max) | old / new | medians of the runs, old | new | min old - max new median | larger spread of medians | larger min-max |",
           "|---|---|---|---|---|---|---|---|---|"]
    for r in recs:
        o, w = r["old"], r["new"]
        out.append("| %s, 2^%d | %s (%s-%s) | %s (%s-%s) | %.2f | %s | %s | %s | %s | %s |" % (
            r["curve"], r["keys"].bit_length() - 1, ms(o["s_median"]), ms(o["s_min"]), ms(o["s_max"]), ms(w["s_median"]), ms(w["s_min"]), ms(w["s_max"]),
            r["old_vs_new"], " / ".join(ms(m) for m in o["run_medians"]), " / ".join(ms(m) for m in w["run_medians"]),
            ms(min(o["run_medians"]) - max(w["run_medians"])), ms(r["median_spread_s"]), ms(r["spread_s"])))
    out += ["", "| curve, n | k_wirex | k_decompress | k_g2_parse subgroup test (by difference) | old pair |", "|---|---|---|---|---|"]
    for r in recs:
        k = r["kernel_us_per_key"]
        out.append("| %s, 2^%d | %.4f | %.4f | %.4f | %.4f |" % (r["curve"], r["keys"].bit_length() - 1, k["k_wirex"], k["k_decompress"],
                                                            k["k_g2_parse_subgroup_test_by_difference"], k["old_pair"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="0,1")
    ap.add_argument("--logn", default="16,20")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--markdown", default="", help="also write the DESIGN.md table rows to this file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keys_compressed.json"))
    a = ap.parse_args()
    lib = _lib.load()
    check(lib.bgls_init(0), "init")
    recs = []
    points = [(int(c), int(ln)) for c in a.curves.split(",") for ln in a.logn.split(",")]
    # the first point of a process pays one-off costs (first allocations at each size, the clock's ramp): it is measured once and thrown away
    discarded = measure(lib, points[0][0], points[0][1], a.steps, 1)
    print("discarded first point: " + json.dumps(discarded), file=sys.stderr, flush=True)
    for c, ln in points:
        recs.append(measure(lib, c, ln, a.steps, a.rounds))
        print(json.dumps(recs[-1]), file=sys.stderr, flush=True)
    doc = {"tool": "gpu_keys_compressed", "device": torch.cuda.get_device_name(0), "steps": a.steps, "clock": "default power state, not pinned; host perf_counter and hip events",
           "counters_from": "tools/gpu_keys_compressed.py (this run)", "rounds": a.rounds,
           "discarded_first_point": discarded, "results": recs}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
    if a.markdown:
        with open(a.markdown, "w") as f:
            f.write(markdown(recs))
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
