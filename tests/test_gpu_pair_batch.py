"""GPU tier: bgls_pair_batch / bgls_pair_batch_dev -- n independent CurveSystem.Pair calls in one set of launches -- against bgls_pair item by
item, byte for byte: batch sizes around the ten items of a wave and the thirty sets of a k_miller_sets block, points at infinity, the
generators against GetGT(), an on-curve Q outside the order-r subgroup, the golden pairing rows, an off-curve point in the middle of a
call, the Python mirror with its item-by-item fallback; and the unchanged-behaviour check of the callers that were NOT rerouted (one
final_exp launch per bgls_bb_verify_batch call, gt_out byte-equal to bgls_pair)."""
import ctypes
import json
import os
import random

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ENCODING = -2
SIZES = (1, 10, 11, 61, 129)


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n, fill=0):
    return (ctypes.c_uint8 * max(1, n))(*([fill] * max(1, n)))


def order_of(cid):
    from bgls_amd import Altbn128, Bls12
    return (Altbn128 if cid == 0 else Bls12).GetG1Order()


def gen(lib, cid, fp, group):
    o = out((2 if group == 1 else 4) * fp)
    assert lib.bgls_generator(cid, group, o) == 0
    return bytes(o)


def scale_gen(lib, cid, fp, group, ks):
    size = (2 if group == 1 else 4) * fp
    o = out(len(ks) * size)
    assert lib.bgls_scale_generator(cid, group, B(b"".join(k.to_bytes(32, "big") for k in ks)), len(ks), o) == 0
    raw = bytes(o)
    return [raw[i * size:(i + 1) * size] for i in range(len(ks))]


def pair(lib, cid, fp, g1, g2):
    o = out(12 * fp)
    assert lib.bgls_pair(cid, B(g1), B(g2), o) == 0
    return bytes(o)


def pair_batch(lib, cid, fp, g1s, g2s):
    n, g = len(g1s), 12 * fp
    o = out(n * g, 0xA5)
    rc = lib.bgls_pair_batch(cid, B(b"".join(g1s)), B(b"".join(g2s)), n, o)
    assert rc == 0, (rc, n)
    raw = bytes(o)
    return [raw[i * g:(i + 1) * g] for i in range(n)]


def off_subgroup_g2(curve):
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "subgroup_%s.json" % curve["name"])))
    return [bytes.fromhex(p["pt"]) for p in fix["points"] if p.get("on_twist") and not p.get("in_subgroup") and not p.get("miller_degenerates")]


def gt_one(fp):
    return bytes(12 * fp - 1) + b"\x01"


def random_pairs(lib, cid, fp, n, seed):
    rnd = random.Random(seed)
    q = order_of(cid)
    return (scale_gen(lib, cid, fp, 1, [rnd.randrange(1, q) for _ in range(n)]), scale_gen(lib, cid, fp, 2, [rnd.randrange(1, q) for _ in range(n)]))


@pytest.fixture(scope="module")
def single_pairs():
    """bgls_pair results shared by the tests of this file: {(cid, g1, g2): GT bytes}"""
    return {}


def want_pair(cache, lib, cid, fp, g1, g2):
    key = (cid, g1, g2)
    if key not in cache:
        cache[key] = pair(lib, cid, fp, g1, g2)
    return cache[key]


def test_every_item_equals_pair(gpu_lib, curve, single_pairs):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    g1, g2 = gen(lib, cid, fp, 1), gen(lib, cid, fp, 2)
    inf1, inf2 = bytes(2 * fp), bytes(4 * fp)
    offs = off_subgroup_g2(curve)
    assert offs
    # one pool of pairs for every size: the random ones, then the special ones spliced in at the sizes that hold them
    P, Q = random_pairs(lib, cid, fp, max(SIZES), 31 + cid)
    special = [(inf1, Q[0]), (P[1], inf2), (inf1, inf2), (g1, g2), (P[2], offs[0]), (P[3], offs[-1])]
    gt_ref = want_pair(single_pairs, lib, cid, fp, g1, g2)
    from bgls_amd import Altbn128, Bls12
    assert gt_ref == (Altbn128 if cid == 0 else Bls12).GetGT().raw
    for n in SIZES:
        g1s, g2s = list(P[:n]), list(Q[:n])
        if n >= 10:                                       # the last six slots of the call, so the final one is special too
            for k, (a, b) in enumerate(special):
                g1s[n - 6 + k], g2s[n - 6 + k] = a, b
        else:
            g1s[0], g2s[0] = g1, g2
        got = pair_batch(lib, cid, fp, g1s, g2s)
        for b in range(n):
            assert got[b] == want_pair(single_pairs, lib, cid, fp, g1s[b], g2s[b]), (n, b)
        if n >= 10:
            assert got[n - 6] == got[n - 5] == got[n - 4] == gt_one(fp), n
            assert got[n - 3] == gt_ref and gt_ref != gt_one(fp)
    # every special pair alone and first
    for a, b in special:
        assert pair_batch(lib, cid, fp, [a], [b])[0] == want_pair(single_pairs, lib, cid, fp, a, b)
        assert pair_batch(lib, cid, fp, [a, P[5]], [b, Q[5]])[0] == want_pair(single_pairs, lib, cid, fp, a, b)


def test_golden_pairing_rows(gpu_lib, curve):
    lib, cid, fp, v = gpu_lib, curve["id"], curve["fp"], curve["vec"]
    rows = v["pairings"]
    got = pair_batch(lib, cid, fp, [bytes.fromhex(r["g1"]) for r in rows], [bytes.fromhex(r["g2"]) for r in rows])
    assert [g.hex() for g in got] == [r["gt"] for r in rows]
    pp = v["pairing_product"]
    got = pair_batch(lib, cid, fp, [bytes.fromhex(x) for x in pp["g1s"]], [bytes.fromhex(x) for x in pp["g2s"]])
    acc = got[0]
    for g in got[1:]:
        o = out(12 * fp)
        assert lib.bgls_gt_mul(cid, B(acc), B(g), o) == 0
        acc = bytes(o)
    assert acc.hex() == pp["gt"]


def test_bilinearity_from_one_call(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(41 + cid)
    q = order_of(cid)
    a, x, y = (rnd.randrange(2, q) for _ in range(3))
    P, aP = scale_gen(lib, cid, fp, 1, [x, a * x % q])
    Q, aQ = scale_gen(lib, cid, fp, 2, [y, a * y % q])
    got = pair_batch(lib, cid, fp, [aP, P, P], [Q, aQ, Q])
    assert got[0] == got[1] != got[2]
    o = out(12 * fp)
    assert lib.bgls_gt_pow(cid, B(got[2]), B(a.to_bytes(32, "big")), 0, o) == 0
    assert bytes(o) == got[0]


def test_an_off_curve_point_fails_the_whole_call(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n, g = 11, 12 * fp
    P, Q = random_pairs(lib, cid, fp, n, 43 + cid)
    off1 = bytearray(P[5]); off1[-1] ^= 1
    off2 = bytearray(Q[5]); off2[-1] ^= 1
    big1 = b"\xff" * fp + P[5][fp:]
    for g1s, g2s in ((P[:5] + [bytes(off1)] + P[6:], Q), (P, Q[:5] + [bytes(off2)] + Q[6:]), (P[:5] + [big1] + P[6:], Q),
                     (P[:10] + [bytes(off1)], Q), (P, Q[:10] + [bytes(off2)])):
        o = out(n * g, 0x5A)
        assert lib.bgls_pair_batch(cid, B(b"".join(g1s)), B(b"".join(g2s)), n, o) == ERR_ENCODING
        assert bytes(o) == b"\x5a" * (n * g)
    assert len(pair_batch(lib, cid, fp, P, Q)) == n


def test_device_form_on_a_stream_of_the_callers(gpu_lib, curve):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n, g = 33, 12 * fp
    P, Q = random_pairs(lib, cid, fp, n, 47 + cid)
    P[4], Q[9] = bytes(2 * fp), bytes(4 * fp)
    want = pair_batch(lib, cid, fp, P, Q)
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        d_p = torch.frombuffer(bytearray(b"".join(P)), dtype=torch.uint8).to(dev)
        d_q = torch.frombuffer(bytearray(b"".join(Q)), dtype=torch.uint8).to(dev)
        d_out = torch.full((n * g,), 0xA5, dtype=torch.uint8, device=dev)
    stream.synchronize()
    assert lib.bgls_pair_batch_dev(cid, d_p.data_ptr(), d_q.data_ptr(), n, d_out.data_ptr(), stream.cuda_stream) == 0
    ob = bytes(d_out.cpu().numpy())
    assert [ob[i * g:(i + 1) * g] for i in range(n)] == want
    d_out.fill_(0)
    torch.cuda.synchronize()
    assert lib.bgls_pair_batch_dev(cid, d_p.data_ptr(), d_q.data_ptr(), n, d_out.data_ptr(), None) == 0
    assert bytes(d_out.cpu().numpy()) == ob


def test_poisoned_and_stale_workspaces(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    P, Q = random_pairs(lib, cid, fp, 129, 53 + cid)
    small = pair_batch(lib, cid, fp, P[:3], Q[:3])
    big = pair_batch(lib, cid, fp, P, Q)
    assert big[:3] == small
    assert pair_batch(lib, cid, fp, P[:3], Q[:3]) == small, "behind a larger call"
    for byte in (0x00, 0xFF):
        filled = ctypes.c_uint64(0)
        assert lib.bgls_selftest_fill_workspaces(byte, 0, ctypes.byref(filled)) == 0 and filled.value > 0
        assert pair_batch(lib, cid, fp, P[:3], Q[:3]) == small, "behind fill(0x%02x)" % byte
    assert pair_batch(lib, cid, fp, P, Q) == big


def test_python_mirror(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12
    from bgls_amd.curves import Point
    C = Altbn128 if curve["id"] == 0 else Bls12
    other = Bls12 if curve["id"] == 0 else Altbn128
    rnd = random.Random(59 + curve["id"])
    n = 12
    p1 = [C.GetG1().Mul(rnd.randrange(1, C.GetG1Order())) for _ in range(n)]
    p2 = [C.GetG2().Mul(rnd.randrange(1, C.GetG1Order())) for _ in range(n)]
    p1[2], p2[3] = C.GetG1Infinity(), C.GetG2Infinity()
    want = [C.Pair(a, b) for a, b in zip(p1, p2)]
    assert all(ok for _, ok in want)
    got = C.PairBatch(p1, p2)
    assert len(got) == n and all(g.Equals(w) for g, (w, _) in zip(got, want))
    assert got[2].Equals(C.GetGTIdentity()) and got[3].Equals(C.GetGTIdentity())
    # a foreign point, a G2 point in the G1 list: Pair's (nil, false) for that item, the batch's values beside it
    for bad in (other.GetG1(), C.GetG2(), None):
        q1 = list(p1)
        q1[7] = bad
        mixed = C.PairBatch(q1, p2)
        assert mixed[7] is None and C.Pair(bad, p2[7]) == (None, False)
        assert all(m.Equals(g) for k, (m, g) in enumerate(zip(mixed, got)) if k != 7)
    # an off-curve point fails the C call as a whole: settled item by item
    raw = bytearray(p1[6].raw); raw[-1] ^= 1
    q1 = list(p1)
    q1[6] = Point(C, 1, bytes(raw))
    settled = C.PairBatch(q1, p2)
    assert settled[6] is None
    assert all(s.Equals(g) for k, (s, g) in enumerate(zip(settled, got)) if k != 6)


def test_the_existing_callers_were_not_rerouted(gpu_lib, curve):
    """with profiling on, one bgls_bb_verify_batch call reports exactly one final_exp launch, and its gt_out is byte-equal to bgls_pair"""
    import test_gpu_bbsigs as bb
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 13
    it = bb.make_items(lib, cid, fp, n, 61 + cid)
    it["m"][4] ^= 1
    ms, cnt = ctypes.c_double(0), ctypes.c_ulonglong(0)
    assert lib.bgls_profile_enable(1) == 0
    try:
        rc, verdicts, gts = bb.run(lib, cid, fp, it)
        assert lib.bgls_profile_get(b"final_exp", ctypes.byref(ms), ctypes.byref(cnt)) == 0
    finally:
        assert lib.bgls_profile_enable(0) == 0
    assert cnt.value == 1 and ms.value > 0
    assert rc == n - 1 and verdicts == [int(b != 4) for b in range(n)]
    for b in range(n):
        q = bb.stepwise_q(lib, cid, fp, it["key"][b], it["r"][b], it["m"][b])
        assert gts[b] == pair(lib, cid, fp, it["sig"][b], q), b
    # the new calls use the same stage names: one miller and one final_exp launch sequence per call
    P, Q = random_pairs(lib, cid, fp, n, 67 + cid)
    assert lib.bgls_profile_enable(1) == 0
    try:
        pair_batch(lib, cid, fp, P, Q)
        counts = {}
        for stage in (b"miller", b"final_exp", b"epilogue"):
            assert lib.bgls_profile_get(stage, ctypes.byref(ms), ctypes.byref(cnt)) == 0
            counts[stage] = cnt.value
    finally:
        assert lib.bgls_profile_enable(0) == 0
    assert counts == {b"miller": 1, b"final_exp": 1, b"epilogue": 1 if cid == 1 else 0}
