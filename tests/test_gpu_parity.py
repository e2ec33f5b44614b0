"""GPU tier: the HIP path, called through the C ABI, against the committed golden fixtures and
against the oracle on seeded inputs.  Bit-exact everywhere (integer arithmetic)."""
import ctypes
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offsets(msgs):
    off = (ctypes.c_uint64 * (len(msgs) + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        off[i] = acc
        acc += len(m)
    off[len(msgs)] = acc
    return off


def hash_batch(lib, cid, n_fp, msgs):
    o = out(len(msgs) * 2 * n_fp)
    rc = lib.bgls_hash_to_g1(cid, B(b"".join(msgs)), offsets(msgs), len(msgs), o)
    assert rc == 0, rc
    raw = bytes(o)
    return [raw[i * 2 * n_fp:(i + 1) * 2 * n_fp] for i in range(len(msgs))]


def test_hash_to_g1_reference_kats(gpu_lib, curve, kat):
    """The reference's own vectors (curves/testcases/*.dat, altbn128_test.go:16-21, bls12_test.go:57-67)."""
    rows = kat[curve["name"]] + curve["vec"]["h2c"]
    msgs = [bytes.fromhex(r["msg"]) for r in rows]
    got = hash_batch(gpu_lib, curve["id"], curve["fp"], msgs)
    for g, r in zip(got, rows):
        assert g.hex() == r["point"]


def test_hash_to_g1_random_vs_oracle(gpu_lib, curve, kat):
    """Batches >= 256 take the compacting-round / staged kernels; the reference KATs ride along so that
    those kernels are pinned by the reference's own vectors too."""
    rnd = random.Random(101)
    msgs = [rnd.randbytes(rnd.choice((0, 1, 5, 32, 64, 64, 64, 135, 136, 300))) for _ in range(300)]
    rows = kat[curve["name"]] + curve["vec"]["h2c"]
    msgs += [bytes.fromhex(r["msg"]) for r in rows]
    got = hash_batch(gpu_lib, curve["id"], curve["fp"], msgs)
    for g, m in zip(got[:300], msgs[:300]):
        assert g == coracle.hash_to_g1(curve["id"], m)
    for g, r in zip(got[300:], rows):
        assert g.hex() == r["point"]
    # the exponentiation-tested rounds (BGLS_H2C=rounds) are exercised by test_alternate_kernel_paths_agree
    # a long tail of tries / all three SW branches: 4096 more messages against the oracle
    many = [rnd.randbytes(64) for _ in range(4096)]
    got = hash_batch(gpu_lib, curve["id"], curve["fp"], many)
    for i in range(0, 4096, 7):
        assert got[i] == coracle.hash_to_g1(curve["id"], many[i])


def test_hash_to_g1_large_batch_schedule(gpu_lib):
    """alt-bn128 batches of 2^17 messages and more test one counter per message and round while most messages are still
    open (k_hash.hip h2c_bn): same points as the oracle on a strided sample (about one message in sixteen of it needs five
    tries or more, i.e. reaches the later rounds), and the same bytes as the small-batch schedule on the first 4096."""
    cid, fp = 0, 32
    rnd = random.Random(1717)
    n = (1 << 17) + 77
    blob = rnd.randbytes(64 * n)
    offs = (ctypes.c_uint64 * (n + 1))(*range(0, 64 * (n + 1), 64))
    o = out(n * 2 * fp)
    assert gpu_lib.bgls_hash_to_g1(cid, B(blob), offs, n, o) == 0
    got = bytes(o)
    small = hash_batch(gpu_lib, cid, fp, [blob[64 * i:64 * i + 64] for i in range(4096)])
    assert b"".join(small) == got[:4096 * 2 * fp]
    for i in list(range(0, n, 997)) + [n - 1, n - 2, 1 << 16, (1 << 17) - 1, 1 << 17]:
        assert got[2 * fp * i:2 * fp * (i + 1)] == coracle.hash_to_g1(cid, blob[64 * i:64 * i + 64]), i


def test_generators(gpu_lib, curve, kat):
    cid, n = curve["id"], curve["fp"]
    g1, g2 = out(2 * n), out(4 * n)
    assert gpu_lib.bgls_generator(cid, 1, g1) == 0 and gpu_lib.bgls_generator(cid, 2, g2) == 0
    row = curve["vec"]["pairings"][3]
    assert bytes(g1).hex() == row["g1"] and bytes(g2).hex() == row["g2"]
    if cid == 0:
        assert bytes(g2).hex() == kat["altbn128_g2_generator"]      # altbn128_test.go:26-38
    assert gpu_lib.bgls_point_check(cid, 1, g1) == 1 and gpu_lib.bgls_point_check(cid, 2, g2) == 1
    bad = bytearray(bytes(g1)); bad[-1] ^= 1
    assert gpu_lib.bgls_point_check(cid, 1, B(bad)) == 0
    assert gpu_lib.bgls_point_check(cid, 1, B(b"\xff" * (2 * n))) == 0   # coordinate >= q


def test_pair_and_product_golden(gpu_lib, curve):
    cid, n, v = curve["id"], curve["fp"], curve["vec"]
    for row in v["pairings"]:
        o = out(12 * n)
        assert gpu_lib.bgls_pair(cid, B(bytes.fromhex(row["g1"])), B(bytes.fromhex(row["g2"])), o) == 0
        assert bytes(o).hex() == row["gt"]
    pp = v["pairing_product"]
    o = out(12 * n)
    assert gpu_lib.bgls_pairing_product(cid, B(b"".join(map(bytes.fromhex, pp["g1s"]))), B(b"".join(map(bytes.fromhex, pp["g2s"]))),
                                        len(pp["g1s"]), o) == 0
    assert bytes(o).hex() == pp["gt"]
    # TestPairingProd (curves/curve_test.go:143-165): product == sequential GT multiplies of Pair
    acc = None
    for a, b in zip(pp["g1s"], pp["g2s"]):
        e = out(12 * n)
        gpu_lib.bgls_pair(cid, B(bytes.fromhex(a)), B(bytes.fromhex(b)), e)
        if acc is None:
            acc = bytes(e)
        else:
            t = out(12 * n)
            assert gpu_lib.bgls_gt_mul(cid, B(acc), e, t) == 0
            acc = bytes(t)
    assert acc.hex() == pp["gt"]
    one = out(12 * n)
    gpu_lib.bgls_gt_identity(cid, one)
    e = out(12 * n)
    assert gpu_lib.bgls_pairing_product(cid, None, None, 0, e) == 0 and bytes(e) == bytes(one)


def test_pairing_product_random_vs_oracle(gpu_lib, curve):
    cid, n = curve["id"], curve["fp"]
    rnd = random.Random(33)
    g1 = bytes.fromhex(curve["vec"]["pairings"][3]["g1"])
    g2 = bytes.fromhex(curve["vec"]["pairings"][3]["g2"])
    N = 150
    g1s = b"".join(coracle.scale_point(cid, 1, g1, rnd.randrange(1, 1 << 250)) for _ in range(N))
    g2s = b"".join(coracle.scale_point(cid, 2, g2, rnd.randrange(1, 1 << 250)) for _ in range(N))
    o = out(12 * n)
    assert gpu_lib.bgls_pairing_product(cid, B(g1s), B(g2s), N, o) == 0
    assert bytes(o) == coracle.pairing_product(cid, g1s, g2s, N, threads=8)


def test_aggregate_and_scale_points(gpu_lib, curve):
    cid, n, v = curve["id"], curve["fp"], curve["vec"]
    for grp, key, size in ((1, "sum_g1", 2 * n), (2, "sum_g2", 4 * n)):
        pts = [bytes.fromhex(x) for x in v[key]["pts"]]
        o = out(size)
        assert gpu_lib.bgls_aggregate_points(cid, grp, B(b"".join(pts)), len(pts), o) == 0
        assert bytes(o).hex() == v[key]["sum"]
        # P + P (doubling branch), P + (-P) = infinity, P + infinity, single point, empty
        o = out(size); gpu_lib.bgls_point_add(cid, grp, B(pts[0]), B(pts[5]), o)
        assert bytes(o) == coracle.aggregate_points(cid, grp, pts[0] + pts[5], 2)
        o = out(size); gpu_lib.bgls_point_add(cid, grp, B(pts[1]), B(pts[6]), o)
        assert bytes(o) == bytes(size)
        o = out(size); gpu_lib.bgls_point_add(cid, grp, B(pts[2]), B(bytes(size)), o)
        assert bytes(o) == pts[2]
        o = out(size); gpu_lib.bgls_aggregate_points(cid, grp, B(pts[3]), 1, o)
        assert bytes(o) == pts[3]
        o = out(size); assert gpu_lib.bgls_aggregate_points(cid, grp, None, 0, o) == 0 and bytes(o) == bytes(size)
        # ragged larger sums (tree passes with a partial last chunk)
        rnd = random.Random(size)
        for N in (17, 257, 1000):
            many = [coracle.scale_point(cid, grp, pts[0], rnd.randrange(1, 1 << 64)) for _ in range(N)]
            o = out(size)
            assert gpu_lib.bgls_aggregate_points(cid, grp, B(b"".join(many)), N, o) == 0
            assert bytes(o) == coracle.aggregate_points(cid, grp, b"".join(many), N)
    for grp, key, size in ((1, "scale_g1", 2 * n), (2, "scale_g2", 4 * n)):
        rows = [r for r in v[key] if abs(int(r["k"])) < 1 << 256]
        pts = b"".join(bytes.fromhex(r["pt"]) for r in rows)
        ks = b"".join(abs(int(r["k"])).to_bytes(32, "big") for r in rows)
        sg = bytes(1 if int(r["k"]) < 0 else 0 for r in rows)
        o = out(size * len(rows))
        assert gpu_lib.bgls_scale_points(cid, grp, B(pts), B(ks), B(sg), len(rows), o) == 0
        for i, r in enumerate(rows):
            assert bytes(o)[i * size:(i + 1) * size].hex() == r["out"], r["k"]
        # nil factor => copy
        o = out(size)
        gpu_lib.bgls_scale_points(cid, grp, B(bytes.fromhex(rows[0]["pt"])), B(bytes(32)), B(b"\x02"), 1, o)
        assert bytes(o).hex() == rows[0]["pt"]


def run_agg(lib, cid, case):
    keys = [bytes.fromhex(k) for k in case["keys"]]
    msgs = [bytes.fromhex(m) for m in case["msgs"]]
    if len(keys) != len(msgs):
        return 0                     # length check lives in the host mirror (bgls/bgls.go:95-97)
    return lib.bgls_verify_aggregate(cid, B(bytes.fromhex(case["sig"])), B(b"".join(keys)), B(b"".join(msgs)), offsets(msgs),
                                     len(keys), 1 if case["allow_dups"] else 0)


def test_verify_aggregate_golden_cases(gpu_lib, curve):
    """bgls/bgls_test.go:40-77 accept/reject matrix, fixed vectors."""
    for case in curve["vec"]["aggregate_cases"]:
        assert (run_agg(gpu_lib, curve["id"], case) == 1) == case["expect"], case["name"]


def test_verify_multi_golden_cases(gpu_lib, curve):
    """bgls/blsKosk_test.go:35-64 accept/reject matrix, fixed vectors."""
    cid = curve["id"]
    for case in curve["vec"]["multi_cases"]:
        keys = b"".join(map(bytes.fromhex, case["keys"]))
        msg = bytes.fromhex(case["msg"])
        rc = gpu_lib.bgls_verify_multi(cid, B(bytes.fromhex(case["sig"])), B(keys), len(case["keys"]), B(msg), len(msg))
        assert (rc == 1) == case["expect"], case["name"]


def make_instance(lib, cid, n_fp, n, seed, msg_len=64):
    """Valid n-signer aggregate instance built with the engine itself (keys, hashes, signatures on the GPU)."""
    rnd = random.Random(seed)
    msgs = [rnd.randbytes(msg_len) for _ in range(n)]
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n)]
    kb = b"".join(s.to_bytes(32, "big") for s in sks)
    g2 = out(4 * n_fp); lib.bgls_generator(cid, 2, g2)
    keys = out(n * 4 * n_fp)
    assert lib.bgls_scale_points(cid, 2, B(bytes(g2) * n), B(kb), None, n, keys) == 0
    hs = b"".join(hash_batch(lib, cid, n_fp, msgs))
    sigs = out(n * 2 * n_fp)
    assert lib.bgls_scale_points(cid, 1, B(hs), B(kb), None, n, sigs) == 0
    agg = out(2 * n_fp)
    assert lib.bgls_aggregate_points(cid, 1, sigs, n, agg) == 0
    return bytes(agg), bytes(keys), msgs


def test_verify_aggregate_random_vs_oracle(gpu_lib, curve):
    cid, n_fp = curve["id"], curve["fp"]
    for n, seed in ((1, 1), (7, 2), (64, 3), (200, 4)):
        agg, keys, msgs = make_instance(gpu_lib, cid, n_fp, n, seed)
        assert coracle.verify_aggregate(cid, agg, keys, msgs, threads=8) == 1       # oracle agrees the instance is valid
        assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(b"".join(msgs)), offsets(msgs), n, 0) == 1
        bad = list(msgs); bad[n // 2] = bytes([bad[n // 2][0] ^ 1]) + bad[n // 2][1:]
        assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(b"".join(bad)), offsets(bad), n, 0) == 0
        assert coracle.verify_aggregate(cid, agg, keys, bad, threads=8) == 0
        if n > 1:
            dup = list(msgs); dup[-1] = dup[0]
            assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(b"".join(dup)), offsets(dup), n, 0) == 0


def test_large_batch_properties(gpu_lib, curve):
    """Size-independent properties at a size the oracle would take minutes for: a valid instance
    verifies, one flipped bit anywhere rejects, and sharding the batch (device API, partial Miller
    products combined like the multi-GPU path) gives the same verdict and the same GT bytes."""
    import torch
    cid, n_fp = curve["id"], curve["fp"]
    n = 4096
    agg, keys, msgs = make_instance(gpu_lib, cid, n_fp, n, 77)
    blob = b"".join(msgs)
    assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(blob), offsets(msgs), n, 0) == 1
    flipped = bytearray(blob); flipped[len(blob) // 3] ^= 0x10
    assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(bytes(flipped)), offsets(msgs), n, 0) == 0
    dev = torch.device("cuda:0")
    t_keys = torch.frombuffer(bytearray(keys), dtype=torch.uint8).to(dev)
    t_msgs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
    t_sig = torch.frombuffer(bytearray(agg), dtype=torch.uint8).to(dev)
    gtb = 12 * n_fp
    verdicts, gts = [], []
    for shards in (1, 2, 5):
        parts = torch.zeros(shards * gtb, dtype=torch.uint8, device=dev)
        flags = torch.zeros(1, dtype=torch.int32, device=dev)
        bounds = [n * s // shards for s in range(shards + 1)]
        for s in range(shards):
            lo, hi = bounds[s], bounds[s + 1]
            rc = gpu_lib.bgls_miller_product_dev(cid, t_sig.data_ptr() if s == 0 else None, t_keys.data_ptr() + lo * 4 * n_fp,
                                                 t_msgs.data_ptr() + lo * 64, 64, 64, hi - lo, 1, parts.data_ptr() + s * gtb,
                                                 flags.data_ptr(), None)
            assert rc == 0
        verdicts.append(gpu_lib.bgls_final_verify_dev(cid, parts.data_ptr(), shards, flags.data_ptr(), None))
        torch.cuda.synchronize()
        acc = bytes(parts[:gtb].cpu().numpy())
        for s in range(1, shards):
            acc = coracle.gt_mul(cid, acc, bytes(parts[s * gtb:(s + 1) * gtb].cpu().numpy()))
        gts.append(acc)
    assert verdicts == [1, 1, 1]
    assert gts[0] == gts[1] == gts[2]          # partial products are canonical: identical bytes for any sharding
    assert coracle.final_exp(cid, gts[0]) == bytes(383 if cid == 0 else 575) + b"\x01"


def test_multisig_large_and_device_api(gpu_lib, curve):
    import torch
    cid, n_fp = curve["id"], curve["fp"]
    n = 3000
    rnd = random.Random(5)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n)]
    kb = b"".join(s.to_bytes(32, "big") for s in sks)
    g2 = out(4 * n_fp); gpu_lib.bgls_generator(cid, 2, g2)
    keys = out(n * 4 * n_fp)
    assert gpu_lib.bgls_scale_points(cid, 2, B(bytes(g2) * n), B(kb), None, n, keys) == 0
    msg = b"\x01" + rnd.randbytes(64)
    h = hash_batch(gpu_lib, cid, n_fp, [msg])[0]
    sig = coracle.scale_point(cid, 1, h, sum(sks) % (1 << 255))        # sum(sk) < 2^262; keep it simple: reduce below
    order = 21888242871839275222246405745257275088548364400416034343698204186575808495617 if cid == 0 else \
        52435875175126190479447740508185965837690552500527637822603658699938581184513
    sig = coracle.scale_point(cid, 1, h, sum(sks) % order)
    assert gpu_lib.bgls_verify_multi(cid, B(sig), keys, n, B(msg), len(msg)) == 1
    assert coracle.verify_multi(cid, sig, bytes(keys), n, msg) == 1
    assert gpu_lib.bgls_verify_multi(cid, B(sig), keys, n - 1, B(msg), len(msg)) == 0
    dev = torch.device("cuda:0")
    t_keys = torch.frombuffer(bytearray(bytes(keys)), dtype=torch.uint8).to(dev)
    t_sig = torch.frombuffer(bytearray(sig), dtype=torch.uint8).to(dev)
    t_msg = torch.frombuffer(bytearray(msg), dtype=torch.uint8).to(dev)
    assert gpu_lib.bgls_verify_multi_dev(cid, t_sig.data_ptr(), t_keys.data_ptr(), n, t_msg.data_ptr(), len(msg), None) == 1
    apk = torch.zeros(4 * n_fp, dtype=torch.uint8, device=dev)
    assert gpu_lib.bgls_aggregate_points_dev(cid, 2, t_keys.data_ptr(), n, apk.data_ptr(), None) == 0
    assert bytes(apk.cpu().numpy()) == coracle.aggregate_points(cid, 2, bytes(keys), n)


def test_bad_encodings_are_errors_not_accepts(gpu_lib, curve):
    cid, n_fp = curve["id"], curve["fp"]
    case = curve["vec"]["aggregate_cases"][0]
    keys = bytearray(b"".join(map(bytes.fromhex, case["keys"])))
    keys[5] ^= 0x40                                   # off-curve key
    msgs = [bytes.fromhex(m) for m in case["msgs"]]
    rc = gpu_lib.bgls_verify_aggregate(cid, B(bytes.fromhex(case["sig"])), B(bytes(keys)), B(b"".join(msgs)), offsets(msgs), len(msgs), 0)
    assert rc == -2
    assert gpu_lib.bgls_verify_aggregate(9, None, None, None, None, 0, 0) < 0


def test_throughput_mode_agrees(gpu_lib, curve):
    """bgls_set_throughput_mode tells the engine that several verifications are in flight: no fork onto the side stream, the
    60-pairing block form and no producer priority even for a batch that is one round of blocks.  Same golden GT bytes, same
    verdicts, same canonical partial-product bytes as the default mode."""
    import torch
    cid, n_fp = curve["id"], curve["fp"]
    lib = gpu_lib
    pp = curve["vec"]["pairing_product"]
    g1s = b"".join(map(bytes.fromhex, pp["g1s"])); g2s = b"".join(map(bytes.fromhex, pp["g2s"]))
    dev = torch.device("cuda:0")
    n = 1000
    agg, keys, msgs = make_instance(lib, cid, n_fp, n, 555)
    t_keys = torch.frombuffer(bytearray(keys), dtype=torch.uint8).to(dev)
    t_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
    t_sig = torch.frombuffer(bytearray(agg), dtype=torch.uint8).to(dev)
    gtb = 12 * n_fp
    parts = {}
    try:
        for mode in (0, 1, 2):                                       # 2: one stream, the lone verification's launch shapes (stage timing)
            assert lib.bgls_set_throughput_mode(mode) == 0
            o = out(gtb)
            assert lib.bgls_pairing_product(cid, B(g1s), B(g2s), len(pp["g1s"]), o) == 0
            assert bytes(o).hex() == pp["gt"]
            for case in curve["vec"]["aggregate_cases"]:
                assert (run_agg(lib, cid, case) == 1) == case["expect"], (mode, case["name"])
            for with_sig in (True, False):
                part = torch.zeros(gtb, dtype=torch.uint8, device=dev)
                flags = torch.zeros(1, dtype=torch.int32, device=dev)
                assert lib.bgls_miller_product_dev(cid, t_sig.data_ptr() if with_sig else None, t_keys.data_ptr(), t_msgs.data_ptr(), 64, 64, n, 1,
                                                   part.data_ptr(), flags.data_ptr(), None) == 0
                if with_sig:
                    assert lib.bgls_final_verify_dev(cid, part.data_ptr(), 1, flags.data_ptr(), None) == 1
                torch.cuda.synchronize()
                parts[(mode, with_sig)] = bytes(part.cpu().numpy())
    finally:
        lib.bgls_set_throughput_mode(0)
    assert parts[(0, True)] == parts[(1, True)] == parts[(2, True)] and parts[(0, False)] == parts[(1, False)] == parts[(2, False)]
    # the partial product without the signature pair is the oracle's product of Miller values over the hash points
    hs = b"".join(coracle.hash_to_g1(cid, m) for m in msgs[:40])
    part = torch.zeros(gtb, dtype=torch.uint8, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    assert lib.bgls_miller_product_dev(cid, None, t_keys.data_ptr(), t_msgs.data_ptr(), 64, 64, 40, 1, part.data_ptr(), flags.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert coracle.final_exp(cid, bytes(part.cpu().numpy())) == coracle.final_exp(cid, coracle.miller_product(cid, hs, keys[:40 * 4 * n_fp], 40))


def test_randomised_sizes_and_corruptions(gpu_lib, curve):
    """Ragged batch sizes around every kernel's tile boundaries (60/64 pairings per block, 6 per group, 256-message
    hashing threshold, reduction fan-in 4): valid instances verify, any single corruption rejects, and the
    pairing product equals the oracle's bytes."""
    cid, n_fp = curve["id"], curve["fp"]
    rnd = random.Random(2026 + cid)
    sizes = [1, 2, 5, 6, 7, 59, 60, 61, 63, 64, 65, 119, 120, 121, 255, 256, 257, 600, 641] + [rnd.randrange(1, 1500) for _ in range(6)]
    for n in sizes:
        agg, keys, msgs = make_instance(gpu_lib, cid, n_fp, n, 9000 + n, msg_len=rnd.choice((8, 32, 64, 100)))   # >= 8 bytes: duplicates would (correctly) reject
        blob = b"".join(msgs)
        assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(blob), offsets(msgs), n, 0) == 1, n
        which = rnd.randrange(3)
        if which == 0:                                    # flip one message bit
            bad = bytearray(blob); bad[rnd.randrange(len(bad))] ^= 1 << rnd.randrange(8)
            r = gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(bytes(bad)), offsets(msgs), n, 1)
        elif which == 1 and n > 1:                        # swap two keys
            i, k = rnd.sample(range(n), 2)
            kk = bytearray(keys); s = 4 * n_fp
            kk[i * s:(i + 1) * s], kk[k * s:(k + 1) * s] = keys[k * s:(k + 1) * s], keys[i * s:(i + 1) * s]
            r = gpu_lib.bgls_verify_aggregate(cid, B(agg), B(bytes(kk)), B(blob), offsets(msgs), n, 0)
        else:                                             # signature of a different instance
            other, _, _ = make_instance(gpu_lib, cid, n_fp, 1, 77, msg_len=8)
            r = gpu_lib.bgls_verify_aggregate(cid, B(other), B(keys), B(blob), offsets(msgs), n, 0)
        assert r == 0, (n, which)
    # pairing products of ragged sizes against the oracle
    g1 = bytes.fromhex(curve["vec"]["pairings"][3]["g1"]); g2 = bytes.fromhex(curve["vec"]["pairings"][3]["g2"])
    for n in (2, 7, 61, 64, 65, 130):
        g1s = b"".join(coracle.scale_point(cid, 1, g1, rnd.randrange(1, 1 << 200)) for _ in range(n))
        g2s = b"".join(coracle.scale_point(cid, 2, g2, rnd.randrange(1, 1 << 200)) for _ in range(n))
        o = out(12 * n_fp)
        assert gpu_lib.bgls_pairing_product(cid, B(g1s), B(g2s), n, o) == 0
        assert bytes(o) == coracle.pairing_product(cid, g1s, g2s, n, threads=8), n


def test_duplicate_scan_across_shards(gpu_lib):
    """bgls_duplicate_scan_dev: exact duplicate detection over device-resident messages -- the multi-GPU path's global
    scan.  A duplicate that straddles two shards escapes both per-shard scans and is caught by the scan over all messages;
    messages that differ in one bit anywhere (first/last byte) are not duplicates."""
    import torch
    dev = torch.device("cuda:0")
    rnd = random.Random(77)
    n, ln = 5000, 64
    msgs = [rnd.randbytes(ln) for _ in range(n)]
    near = bytearray(msgs[10]); near[-1] ^= 1
    msgs[4000] = bytes(near)                                   # one-bit neighbour, not a duplicate
    def scan(buf, count, stride=ln, length=ln):
        t = torch.frombuffer(bytearray(buf), dtype=torch.uint8).to(dev)
        f = torch.zeros(1, dtype=torch.int32, device=dev)
        assert gpu_lib.bgls_duplicate_scan_dev(t.data_ptr(), length, stride, count, f.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return int(f.item())
    assert scan(b"".join(msgs), n) == 0
    msgs[4321] = msgs[123]                                     # shards [0, 2500) and [2500, 5000)
    assert scan(b"".join(msgs[:2500]), 2500) == 0 and scan(b"".join(msgs[2500:]), 2500) == 0
    assert scan(b"".join(msgs), n) & 1
    # stride > length: only the first `length` bytes of each slot count
    assert scan(b"".join(m[:32] + bytes(32) for m in msgs), n, 64, 32) & 1
    assert scan(b"".join(msgs[:2]), 2) == 0 and scan(msgs[0] + msgs[0], 2) & 1 and scan(msgs[0], 1) == 0


def test_bucketed_digest_scan_agrees_with_the_full_scan(gpu_lib):
    """Round 5: the multi-GPU duplicate rule with the digest scan itself sharded.  Rank r scans the digests whose first byte is
    r mod N (bgls_duplicate_scan_bucket_dev); over the N buckets exactly one scan reports the duplicate, none reports anything on a
    clean batch, every digest belongs to one bucket -- and a bucket that overflows its table (records that all share one first
    byte: not digests) reports a hit instead of missing a duplicate."""
    import hashlib
    import torch
    dev = torch.device("cuda:0")
    rnd = random.Random(91)
    n, ln = 40000, 64
    msgs = [rnd.randbytes(ln) for _ in range(n)]
    t_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
    dig = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
    assert gpu_lib.bgls_message_digests_dev(t_msgs.data_ptr(), ln, ln, n, dig.data_ptr(), None) == 0
    torch.cuda.synchronize()
    raw = bytes(dig.cpu().numpy())
    for i in (0, 777, n - 1):
        assert raw[16 * i:16 * i + 16] == hashlib.blake2b(msgs[i]).digest()[:16]

    def buckets(t, count, nb, rl=16):
        out = []
        for b in range(nb):
            f = torch.zeros(1, dtype=torch.int32, device=dev)
            assert gpu_lib.bgls_duplicate_scan_bucket_dev(t.data_ptr(), rl, rl, count, b, nb, f.data_ptr(), None) == 0
            torch.cuda.synchronize()
            out.append(int(f.item()) & 1)
        return out
    for nb in (1, 2, 3, 8):
        assert buckets(dig, n, nb) == [0] * nb
    d2 = dig.clone()
    d2[16 * 31234:16 * 31234 + 16] = d2[16 * 99:16 * 99 + 16]            # digest 99 again at 31234 (a duplicate message, or a collision)
    torch.cuda.synchronize()
    for nb in (1, 2, 3, 8):
        got = buckets(d2, n, nb)
        assert sum(got) == 1 and got[raw[16 * 99] % nb] == 1, (nb, got)
    assert gpu_lib.bgls_duplicate_scan_bucket_dev(d2.data_ptr(), 16, 16, n, 8, 8, None, None) < 0      # bucket out of range / NULL word
    f = torch.zeros(1, dtype=torch.int32, device=dev)
    assert gpu_lib.bgls_duplicate_scan_bucket_dev(d2.data_ptr(), 16, 16, n, 3, 2, f.data_ptr(), None) < 0
    # 40 000 distinct records with the same first byte all land in bucket 1 of 8, whose table is sized for twice a fair share:
    # the scan must say "hit" (undecided -> the caller's exact scan), never a silent miss
    same = bytearray(b"".join(b"\x09" + rnd.randbytes(15) for _ in range(n)))
    t_same = torch.frombuffer(same, dtype=torch.uint8).to(dev)
    got = buckets(t_same, n, 8)
    assert got[1] == 1 and sum(got) == 1


def test_bucketed_digest_scan_at_adversarial_scale(gpu_lib):
    """Advice r5 (medium): a signer can grind messages until every digest's first byte falls into ONE rank's bucket.  With 2^20 such records
    and 16 buckets that bucket's table (sized for twice a fair share) is 4x over-subscribed: round 5's kernel walked the whole table per
    insert -- about 10^12 probes, a hung GPU.  The scan is bounded (1024 probes, and every thread leaves once the flag is up): it must come
    back at once with "hit" (undecided -> the exact scan), the other buckets with nothing, and a fair 2^20-digest batch must still pass."""
    import time
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    n = 1 << 20
    rs = np.random.RandomState(5)
    recs = rs.randint(0, 256, size=(n, 16), dtype=np.uint8)
    fair = torch.from_numpy(recs.copy()).to(dev)
    recs[:, 0] = 16 * rs.randint(0, 16, size=n).astype(np.uint8) + 5          # every first byte is 5 mod 16
    evil = torch.from_numpy(recs).to(dev)
    f = torch.zeros(1, dtype=torch.int32, device=dev)

    def scan(t, b, nb):
        f.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert gpu_lib.bgls_duplicate_scan_bucket_dev(t.data_ptr(), 16, 16, n, b, nb, f.data_ptr(), None) == 0
        torch.cuda.synchronize()
        return int(f.item()) & 1, time.perf_counter() - t0
    scan(fair, 0, 16)                                    # first call: workspace allocation
    for b in (0, 5, 15):
        hit, dt = scan(fair, b, 16)
        assert hit == 0 and dt < 0.25, (b, hit, dt)
    hit, dt = scan(evil, 5, 16)
    assert hit == 1 and dt < 0.25, (hit, dt)             # round 5: did not return
    for b in (0, 4, 6):
        hit, dt = scan(evil, b, 16)
        assert hit == 0 and dt < 0.25, (b, hit, dt)
    # the exact scan (one bucket) of the same records is unbounded by design and still exact: no duplicate among them
    hit, dt = scan(evil, 0, 1)
    assert hit == 0 and dt < 1.0, (hit, dt)


def test_bench_two_ranks_share_one_gpu():
    """The N > 1 path of bench.py end to end on real kernels: two ranks on cuda:0 exchanging over gloo
    (BGLS_BENCH_SHARE_GPU=1) -- shard ranges, global duplicate scan, partial + status all-gather, final verification and,
    with --full, the tampered-message gate and the other records all run; only the numbers are meaningless."""
    import json, os, socket, subprocess, sys
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ); env["BGLS_BENCH_SHARE_GPU"] = "1"
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                          "--signers", "8192", "--no-cpu-baseline", "--reps", "1", "--full"], env=env, capture_output=True, text=True, timeout=900, cwd=root)
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) == 1, (out.stdout[-800:], out.stderr[-1500:])
    assert out.stdout.rstrip().splitlines()[-1] == lines[0] and len(lines[0]) < 4096      # the compact record is the LAST line
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "strong" and d["config"]["signers_per_gpu"] == 4096
    assert d["roofline"]["frac"] > 0 and d["collective"]["world"] == 2 and d["collective"]["backend"] == "gloo" and d["collective"]["bytes_per_step"] > 0
    assert d["records"]["bls12_8192"]["value"] > 0 and d["records"]["altbn128_multisig_8192"]["value"] > 0
    # the full per-record detail rides on an earlier line
    det = [l for l in out.stdout.splitlines() if l.startswith("DETAIL {")]
    assert len(det) == 1
    full = json.loads(det[0][len("DETAIL "):])
    other = full["records"]["bls12_8192"]                  # the BLS12-381 record is measured for every N
    assert other["n_gpus"] == 2 and other["value"] > 0 and other["config"]["signers_per_gpu"] == 4096
    ms = full["records"]["altbn128_multisig_8192"]         # config 4 cut over the ranks: partial key sums, one all-gather
    assert ms["n_gpus"] == 2 and ms["value"] > 0 and ms["scaling"] == "strong"


def test_bench_dump_outputs(tmp_path):
    """bench.py --dump-outputs: the last timed step's verdict, status word and partial Miller product land as float .npy files,
    and two runs with the same seeded inputs but different launch shapes (one vs four verifications in flight) dump the same arrays."""
    import json, os, subprocess, sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for in_flight in (1, 4):
        d = tmp_path / ("inflight%d" % in_flight)
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--only", "aggregate", "--signers", "4096", "--steps", "3",
                              "--warmup", "1", "--reps", "1", "--in-flight", str(in_flight), "--no-cpu-baseline", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=root)
        assert out.returncode == 0, (out.stdout[-800:], out.stderr[-1500:])
        rec = json.loads(out.stdout.rstrip().splitlines()[-1])
        assert rec["steps"] == 3 and rec["ms_per_step"] > 0
        dumps.append({f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(d))})
    a, b = dumps
    assert set(a) == {"verdict", "status", "gt_partial"}
    assert a["verdict"].tolist() == [1.0] and a["status"].tolist() == [0.0]
    assert a["gt_partial"].dtype == np.float32 and a["gt_partial"].shape == (12 * 32,) and a["gt_partial"].any()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_bench_plain_run_is_headline_only():
    """bench.py without --full: the headline's figure and nothing else -- no roofline, no CPU baseline, no other records, no
    message-H2D leg -- while value and ms_per_step keep their meaning (signers / median step time)."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--signers", "4096", "--steps", "3", "--warmup", "1",
                          "--reps", "1"], capture_output=True, text=True, timeout=600, cwd=root)
    assert out.returncode == 0, (out.stdout[-800:], out.stderr[-1500:])
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and out.stdout.rstrip().splitlines()[-1] == lines[0]
    rec = json.loads(lines[0])
    assert rec["metric"] == "aggregate-verify signer-pairs/sec" and rec["unit"] == "signer-pairs/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "u32" and rec["steps"] == 3 and rec["warmup"] == 1 and rec["n_gpus"] == 1
    assert rec["ms_per_step"] > 0 and abs(rec["value"] * rec["ms_per_step"] * 1e-3 / 4096 - 1) < 1e-4
    assert rec["roofline"] is None and rec["cpu_baseline"] is None and rec["records"] == {}
    det = [l for l in out.stdout.splitlines() if l.startswith("DETAIL {")]
    assert len(det) == 1
    full = json.loads(det[0][len("DETAIL "):])
    assert "with_message_h2d" not in full and full["roofline"] is None and full["records"] == {}


def test_two_contexts_in_flight(gpu_lib, curve):
    """bgls_select_context + bgls_final_verify_submit_dev / _collect: two verifications enqueued back to back on two
    contexts (own streams, own workspaces) give their own verdicts -- a valid instance and one with a flipped message bit."""
    import torch
    cid, n_fp = curve["id"], curve["fp"]
    n = 700
    agg, keys, msgs = make_instance(gpu_lib, cid, n_fp, n, 4242)
    dev = torch.device("cuda:0")
    blob = b"".join(msgs)
    bad = bytearray(blob); bad[64 * 301 + 7] ^= 4
    t_keys = torch.frombuffer(bytearray(keys), dtype=torch.uint8).to(dev)
    t_sig = torch.frombuffer(bytearray(agg), dtype=torch.uint8).to(dev)
    t_msgs = [torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev), torch.frombuffer(bad, dtype=torch.uint8).to(dev)]
    gtb = 12 * n_fp
    parts = [torch.zeros(gtb, dtype=torch.uint8, device=dev) for _ in range(2)]
    flags = [torch.zeros(1, dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    try:
        for rep in range(2):
            for k in (0, 1):
                assert gpu_lib.bgls_select_context(k) == 0
                assert gpu_lib.bgls_miller_product_dev(cid, t_sig.data_ptr(), t_keys.data_ptr(), t_msgs[k].data_ptr(), 64, 64, n, 1,
                                                       parts[k].data_ptr(), flags[k].data_ptr(), None) == 0
                assert gpu_lib.bgls_final_verify_submit_dev(cid, parts[k].data_ptr(), 1, flags[k].data_ptr(), None) == 0
            assert gpu_lib.bgls_final_verify_submit_dev(cid, parts[1].data_ptr(), 1, flags[1].data_ptr(), None) < 0   # one in flight per context
            got = []
            for k in (0, 1):
                assert gpu_lib.bgls_select_context(k) == 0
                got.append(gpu_lib.bgls_final_verify_collect(cid))
            assert got == [1, 0]
            assert gpu_lib.bgls_final_verify_collect(cid) < 0          # nothing left to collect
        assert gpu_lib.bgls_select_context(99) < 0
    finally:
        gpu_lib.bgls_select_context(0)


def test_batch_beyond_one_launch(gpu_lib, curve):
    """More than 2^16 signers: the Miller stage runs as consecutive 1024-block launches (the signature pair rides on the
    first one, ragged tail on the last).  A valid instance verifies; corrupting a message in the first launch, in the
    last launch or the signature rejects."""
    cid, n_fp = curve["id"], curve["fp"]
    n = 65536 + 64 * 3 + 5
    agg, keys, msgs = make_instance(gpu_lib, cid, n_fp, n, 31337)
    blob = b"".join(msgs)
    off = offsets(msgs)
    assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(blob), off, n, 0) == 1
    for pos in (64 * 10 + 3, 64 * (n - 2) + 1):
        bad = bytearray(blob); bad[pos] ^= 0x40
        assert gpu_lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(bytes(bad)), off, n, 0) == 0
    g1 = out(2 * n_fp); gpu_lib.bgls_generator(cid, 1, g1)
    assert gpu_lib.bgls_verify_aggregate(cid, g1, B(keys), B(blob), off, n, 0) == 0


def test_host_threads_on_their_own_contexts(gpu_lib):
    """Four host threads, each on its own context (bgls_select_context is per thread), verify different instances of both
    curves at once -- valid and tampered, small (latency kernels) and large (batch kernels), aggregate and multi-signature,
    plus hashed-exponent sums: every call answers as it does alone.  ctypes releases the GIL during the calls, so the
    library's context locks, per-device tables and workspaces really are entered concurrently."""
    import threading
    lib = gpu_lib
    jobs = []
    for k, (cid, n_fp, n) in enumerate(((0, 32, 40), (1, 48, 300), (0, 32, 3000), (1, 48, 90))):
        agg, keys, msgs = make_instance(lib, cid, n_fp, n, 9000 + k)
        bad = list(msgs); bad[n // 3] = bytes([bad[n // 3][0] ^ 0x40]) + bad[n // 3][1:]
        jobs.append((cid, n, agg, keys, msgs, bad))
    errors = []

    def work(k):
        try:
            cid, n, agg, keys, msgs, bad = jobs[k]
            assert lib.bgls_select_context(k) == 0
            for it in range(6):
                assert lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(b"".join(msgs)), offsets(msgs), n, 0) == 1, (k, it)
                assert lib.bgls_verify_aggregate(cid, B(agg), B(keys), B(b"".join(bad)), offsets(bad), n, 0) == 0, (k, it)
                t = out(16 * n)
                assert lib.bgls_hae_exponents(cid, B(keys), n, t) == 0
                assert bytes(t) == coracle.blake2xb(keys, 16 * n)
        except Exception as e:                                        # noqa: BLE001 -- reported by the main thread
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    lib.bgls_select_context(0)
    assert not errors, errors


def test_digest_pack_and_packed_scan(gpu_lib):
    """Round 6: the two halves of the all-to-all digest exchange on ONE GPU.  Pack 50 000 digests for N = 2, 3, 8 ranks; every digest
    must sit in its bucket's slot, the rest of a slot is padding of the NEXT bucket, nothing is lost or invented; the scan of a slot
    set finds a planted pair only in its owner's bucket; a slot too small for its share raises the word."""
    import hashlib
    import numpy as np
    import torch
    dev = torch.device("cuda:0")
    n = 50000
    rs = np.random.RandomState(11)
    dig = rs.randint(0, 256, size=(n, 16), dtype=np.uint8)
    dig[:, 1] |= 1                                                    # no real record looks like padding (bytes 1..15 all zero)
    t = torch.from_numpy(dig).to(dev)
    for nb in (2, 3, 8):
        cap = n // nb + n // (4 * nb) + 1024
        out = torch.zeros(nb * cap * 16, dtype=torch.uint8, device=dev)
        w = torch.zeros(1, dtype=torch.int32, device=dev)
        assert gpu_lib.bgls_digest_pack_dev(t.data_ptr(), n, nb, cap, out.data_ptr(), w.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(w.item()) == 0
        o = out.cpu().numpy().reshape(nb, cap, 16)
        seen = 0
        for b in range(nb):
            real = o[b][np.any(o[b][:, 1:] != 0, axis=1)]
            pad = o[b][np.all(o[b][:, 1:] == 0, axis=1)]
            assert np.all(real[:, 0] % nb == b) and np.all(pad[:, 0] == (b + 1) % nb)
            want = dig[dig[:, 0] % nb == b]
            assert sorted(map(bytes, real)) == sorted(map(bytes, want))
            seen += len(real)
        assert seen == n
        # a rank's receive buffer = slot `r` of every rank's send buffer; here: the same rank's slot nb times over would plant duplicates,
        # so build it from ONE copy of slot r and padding
        for r in range(nb):
            recv = torch.from_numpy(np.concatenate([o[r]] + [np.tile(np.array([(r + 1) % nb] + [0] * 15, dtype=np.uint8), (cap, 1))] * (nb - 1))).to(dev)
            w.zero_()
            assert gpu_lib.bgls_duplicate_scan_packed_dev(recv.data_ptr(), nb * cap, r, nb, w.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert int(w.item()) & 1 == 0, (nb, r)
        d2 = dig.copy()
        d2[n - 5] = d2[123]
        t2 = torch.from_numpy(d2).to(dev)
        assert gpu_lib.bgls_digest_pack_dev(t2.data_ptr(), n, nb, cap, out.data_ptr(), w.data_ptr(), None) == 0
        torch.cuda.synchronize()
        o2 = out.cpu().numpy().reshape(nb, cap, 16)
        owner = int(d2[123, 0]) % nb
        for r in range(nb):
            recv = torch.from_numpy(np.ascontiguousarray(o2[r])).to(dev)
            w.zero_()
            assert gpu_lib.bgls_duplicate_scan_packed_dev(recv.data_ptr(), cap, r, nb, w.data_ptr(), None) == 0
            torch.cuda.synchronize()
            assert (int(w.item()) & 1) == (1 if r == owner else 0), (nb, r, owner)
        # a slot smaller than the bucket's share: the word is raised, nothing is written past the slot
        small = n // (2 * nb)
        guard = torch.full((nb * small * 16 + 64,), 0xAB, dtype=torch.uint8, device=dev)
        w.zero_()
        assert gpu_lib.bgls_digest_pack_dev(t.data_ptr(), n, nb, small, guard.data_ptr(), w.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert int(w.item()) & 1 == 1 and bytes(guard[-64:].cpu().numpy()) == b"\xab" * 64
    w = torch.zeros(1, dtype=torch.int32, device=dev)
    assert gpu_lib.bgls_digest_pack_dev(t.data_ptr(), n, 1, 10, t.data_ptr(), w.data_ptr(), None) < 0          # one bucket: nothing to exchange
    assert gpu_lib.bgls_duplicate_scan_packed_dev(t.data_ptr(), n, 2, 2, w.data_ptr(), None) < 0


def test_scale_points_at_exceptional_points_and_scalars(gpu_lib, curve):
    """bgls_scale_points on G1 (k_scale_g1x on BLS12-381: rx_jac1.hpp's windowed chain) where the chain leaves its general addition: the
    order-3 point (0, 2) of BLS12-381 and its negative (table entries at infinity), the fixture's on-curve points outside the subgroup,
    and on the generator the scalars of the host tier's list -- k = j q (the last addition cancels), k = j (q - 2) (it doubles), every
    window-crossing bit length -- under sign bytes 0 and 1.  Expected bytes: the plain affine reference (tests/ec_ref.py), scalars unreduced."""
    import point_cases as pc
    from ec_ref import Curve
    cid, fp = curve["id"], curve["fp"]
    cv = Curve(cid, 1)
    rnd = random.Random(61 + cid)
    items = []                                                             # (point, k)
    for c in pc.mul_cases(cid, 1):
        if c["tag"].startswith("g, "):
            items.append((cv.from_bytes(c["pt"]), c["k"] & ((1 << c["nbits"]) - 1)))
    others = [pt for pt, _, _ in pc.fixture_points(cid, 1) + pc.special_points(cid, 1)]
    if cid == 1:
        assert (0, 2) in others or cv.neg((0, 2)) in others
        others += [pt for pt in ((0, 2), cv.neg((0, 2))) if pt not in others]
    for pt in others:
        for k in [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, (1 << 256) - 1, ORDER_OF[cid], ORDER_OF[cid] - 2] + [rnd.getrandbits(256) for _ in range(12)] + [rnd.getrandbits(128) for _ in range(4)]:
            items.append((pt, k))
    memo = {}
    for sign in (0, 1):
        n = len(items)
        o = out(n * 2 * fp)
        rc = gpu_lib.bgls_scale_points(cid, 1, B(b"".join(cv.to_bytes(pt) for pt, _ in items)), B(b"".join(k.to_bytes(32, "big") for _, k in items)),
                                       B(bytes([sign]) * n), n, o)
        assert rc == 0, rc
        raw = bytes(o)
        for i, (pt, k) in enumerate(items):
            if (pt, k) not in memo:
                memo[(pt, k)] = cv.mul(pt, k)
            want = cv.neg(memo[(pt, k)]) if sign else memo[(pt, k)]
            assert raw[i * 2 * fp:(i + 1) * 2 * fp] == cv.to_bytes(want), (sign, i, hex(k))
            if pt is not None and pt[0] == 0:                              # (0, +-2): order 3, the closed form
                base = cv.neg(pt) if sign else pt
                assert want == [None, base, cv.neg(base)][k % 3]


ORDER_OF = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
            1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}


def test_sign_batch_with_secret_keys_at_the_group_order(gpu_lib, curve):
    """bgls_sign_batch (k_scale_aff_g1x) with the secret keys q, 2 q and q - 2 among ordinary ones: sk H(m) for the integer sk as given --
    infinity, infinity and -2 H(m)"""
    from ec_ref import Curve
    cid, fp = curve["id"], curve["fp"]
    cv = Curve(cid, 1)
    q = ORDER_OF[cid]
    rnd = random.Random(67 + cid)
    n = 70
    sks = [rnd.randrange(1, q) for _ in range(n)]
    for at, k in ((0, q), (31, 2 * q), (32, q - 2), (63, q), (64, q - 2), (69, 2 * q), (5, q + 1), (6, q - 1)):
        sks[at] = k
    msgs = [rnd.randbytes(1 + i % 40) for i in range(n)]
    hs = hash_batch(gpu_lib, cid, fp, msgs)
    sg = out(n * 2 * fp)
    assert gpu_lib.bgls_sign_batch(cid, B(b"".join(k.to_bytes(32, "big") for k in sks)), B(b"".join(msgs)), offsets(msgs), n, sg) == 0
    raw = bytes(sg)
    for i in range(n):
        h = cv.from_bytes(hs[i])
        assert cv.on_curve(h)
        assert raw[i * 2 * fp:(i + 1) * 2 * fp] == cv.to_bytes(cv.mul(h, sks[i])), (i, hex(sks[i]))
    assert raw[:2 * fp] == bytes(2 * fp) and raw[31 * 2 * fp:32 * 2 * fp] == bytes(2 * fp)
    h32 = cv.from_bytes(hs[32])
    assert raw[32 * 2 * fp:33 * 2 * fp] == cv.to_bytes(cv.neg(cv.dbl(h32)))
