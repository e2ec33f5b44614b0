#!/usr/bin/env python3
"""Regenerate tests/golden/h2c_deep_altbn128.json: real 64-byte messages whose alt-bn128 try-and-increment (curves/hash.go:53-77) first
accepts at counter 0, 1, ..., TOP, PER_DEPTH messages per counter, with their try count and point.

A random message first accepts at counter k with probability 2^-(k+1), so the deep rows are MINED: message i is
BLAKE2b-512(SEED || i), the indices are scanned in order in blocks of BLOCK (split over at most 16 worker processes), and the rows of a
depth are the PER_DEPTH smallest indices that reach it -- the same file whatever the number of workers.  The scan asks the C oracle
(oracle/c, oracle_bn_h2c_tries: one Keccak and one square-root exponentiation per try); the Python oracle (oracle/pyref) then computes
every row's point and try count on its own, and the C oracle must give the same bytes.

What the depths are for (bgls_amd/csrc/k_hash.hip): 5 is the first counter of the middle schedule's <32> round, 15 the first of the
wide kernel's second pass, 16 the first of the lean schedule's <32> round.

Measured: TOP = 18 needed 4 blocks (2^20 messages, about 45 us each) and 7 s of wall time on 8 processes.
"""
import hashlib, json, os, sys, time
from concurrent.futures import ProcessPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = b"bgls h2c deep 20261018"
TOP = 18
PER_DEPTH = 2
BLOCK = 1 << 18
WORKERS = min(16, os.cpu_count() or 1)


def message(i):
    return hashlib.blake2b(SEED + i.to_bytes(8, "big"), digest_size=64).digest()


def scan(span):
    """(counter, index) of every message of the span whose first accepting counter is 5 or more, and the first PER_DEPTH of each shallower one"""
    from oracle import coracle
    lo, hi = span
    hits, shallow = [], {}
    for i in range(lo, hi):
        c = coracle.bn_h2c_tries(message(i)) - 1
        if c >= 5:
            hits.append((c, i))
        elif len(shallow.setdefault(c, [])) < PER_DEPTH:
            shallow[c].append(i)
    return hits + [(c, i) for c, v in shallow.items() for i in v]


def main():
    from oracle import coracle
    from oracle.pyref import h2c
    t0 = time.time()
    found = {c: [] for c in range(TOP + 1)}
    blocks = 0
    with ProcessPoolExecutor(max_workers=WORKERS) as ex:
        while any(len(v) < PER_DEPTH for v in found.values()):
            lo = blocks * BLOCK
            step = BLOCK // 64
            for part in ex.map(scan, [(a, a + step) for a in range(lo, lo + BLOCK, step)]):
                for c, i in part:
                    if 0 <= c <= TOP:
                        found[c].append(i)
            blocks += 1
    mined = time.time() - t0
    rows = []
    for c in range(TOP + 1):
        for i in sorted(found[c])[:PER_DEPTH]:
            m = message(i)
            x, y, tries = h2c.altbn_hash_to_g1(m)
            assert tries == c + 1, (i, c, tries)
            pt = x.to_bytes(32, "big") + y.to_bytes(32, "big")
            assert coracle.hash_to_g1(0, m) == pt and coracle.bn_h2c_tries(m) == tries
            rows.append({"index": i, "msg": m.hex(), "counter": c, "tries": tries, "point": pt.hex()})
    out = {"curve": "altbn128", "seed": SEED.decode(), "top": TOP, "rows": rows}
    json.dump(out, open(os.path.join(HERE, "h2c_deep_altbn128.json"), "w"), indent=0)
    print("h2c_deep_altbn128.json: %d rows, %d blocks of %d messages, mined in %.0f s on %d processes" % (len(rows), blocks, BLOCK, mined, WORKERS))


if __name__ == "__main__":
    main()
