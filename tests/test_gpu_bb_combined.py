"""GPU tier: many Boneh-Boyen signatures under one combined check per group (bgls_bb_verify_batch_combined / _dev).  Every group's GT
element byte for byte against bgls_pairing_product over pairs built with the existing calls -- bgls_rlc_coefficients for the rho_b,
bgls_scale_points for rho_b sigma_b, the Q_b of the per-point calls (their batch forms, sampled against stepwise_q), bgls_scale_generator
on (order - s_g mod order) for -s_g g1 -- and the C oracle's
product for the smallest groups; ragged group sizes around the six-pairing padding, the 60-pairing block and the 64-lane wave of
k_bb_rlc_sums (on BLS12-381: the epilogue without its cofactor power); the single-group path; rejection and isolation against the
per-item call; the cancellation pair; edge items; whole-call errors; the device form, a second stream, throughput modes and profile
scopes; 2^12 items with the located fallback; the Python mirrors."""
import ctypes
import random

import pytest

import test_gpu_bbsigs as tb
import test_gpu_multi_sets_combined as mc
from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ENCODING = -2
B, out, gen, make_items, stepwise_q = tb.B, tb.out, tb.gen, tb.make_items, tb.stepwise_q
offs, identity = mc.offs, mc.identity
GROUP_SIZES = [0, 1, 5, 6, 7, 59, 60, 61, 63, 64, 65]
SEED = bytes(range(32))
_ITEMS = {}


def items(lib, cid, fp, n, seed):
    """make_items once per (curve, n, seed); every test works on its own copy"""
    key = (cid, n, seed)
    if key not in _ITEMS:
        _ITEMS[key] = make_items(lib, cid, fp, n, seed)
    return {k: list(v) for k, v in _ITEMS[key].items()}


def packed(it):
    return (B(b"".join(it["sig"])), B(b"".join(r.to_bytes(32, "big") for r in it["r"])), B(b"".join(it["key"])),
            B(b"".join(m.to_bytes(32, "big") for m in it["m"])))


def run_combined(lib, cid, fp, it, groups, seed=SEED, want_gt=True):
    """groups: the list of group sizes, or None for group_off = NULL"""
    n, ng = len(it["sig"]), (1 if groups is None else len(groups))
    v = out(ng)
    gt = out(ng * 12 * fp) if want_gt else None
    rc = lib.bgls_bb_verify_batch_combined(cid, *packed(it), n, None if groups is None else offs(groups), ng, B(seed), v, gt)
    return rc, list(v)[:ng], (bytes(gt)[:ng * 12 * fp] if want_gt else None)


def batch_q(lib, cid, fp, it):
    """Q_b = m_b g2 + U_b + r_b V_b for every item with the per-point calls in their batch forms (bgls_scale_generator, bgls_scale_points,
    bgls_aggregate_sets over the three points of an item); every 16th item, and the last, against stepwise_q's four calls per item"""
    n, G2B = len(it["sig"]), 4 * fp
    mg2 = tb.scale_gen(lib, cid, fp, 2, it["m"])
    rv = out(n * G2B)
    assert lib.bgls_scale_points(cid, 2, B(b"".join(k[G2B:] for k in it["key"])), B(b"".join(r.to_bytes(32, "big") for r in it["r"])), None, n, rv) == 0
    q = out(n * G2B)
    parts = b"".join(mg2[b] + it["key"][b][:G2B] + bytes(rv)[b * G2B:(b + 1) * G2B] for b in range(n))
    assert lib.bgls_aggregate_sets(cid, 2, B(parts), offs([3] * n), n, q) == 0
    qs = [bytes(q)[b * G2B:(b + 1) * G2B] for b in range(n)]
    for b in sorted(set(range(0, n, 16)) | {n - 1}):
        assert qs[b] == stepwise_q(lib, cid, fp, it["key"][b], it["r"][b], it["m"][b]), b
    return qs


def want_gts(lib, cid, fp, it, groups, seed=SEED, oracle_for=()):
    """per group: bgls_pairing_product over (rho_b sigma_b, Q_b) and (-s_g g1, g2), everything from the existing calls"""
    n = len(it["sig"])
    groups = [n] if groups is None else groups
    G1B, G2B = 2 * fp, 4 * fp
    q = tb.order_of(cid)
    r = mc.coefficients(lib, seed, n)
    rs = out(n * G1B)
    assert lib.bgls_scale_points(cid, 1, B(b"".join(it["sig"])), B(b"".join(bytes(16) + r[16 * b:16 * b + 16] for b in range(n))), None, n, rs) == 0
    qs = batch_q(lib, cid, fp, it)
    g2 = gen(lib, cid, fp, 2)
    res, at = [], 0
    for g, c in enumerate(groups):
        if c == 0:
            res.append(identity(fp))
            continue
        s = sum(int.from_bytes(r[16 * b:16 * b + 16], "big") for b in range(at, at + c))
        nsg = tb.scale_gen(lib, cid, fp, 1, [(q - s % q) % q])[0]                             # -s_g g1
        g1s = bytes(rs)[at * G1B:(at + c) * G1B] + nsg
        g2s = b"".join(qs[at:at + c]) + g2
        gt = out(12 * fp)
        assert lib.bgls_pairing_product(cid, B(g1s), B(g2s), c + 1, gt) == 0
        res.append(bytes(gt))
        if g in oracle_for:
            assert coracle.pairing_product(cid, g1s, g2s, c + 1, threads=8) == bytes(gt), g
        at += c
    return b"".join(res)


def per_item(lib, cid, fp, it):
    return tb.run(lib, cid, fp, it, want_gt=False)[1]


def test_ragged_groups(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(1900 + cid)
    groups = list(GROUP_SIZES)
    rnd.shuffle(groups)
    n = sum(groups)                                          # 391 items
    it = items(lib, cid, fp, n, 1901 + cid)
    rc, v, gts = run_combined(lib, cid, fp, it, groups)
    assert rc == len(groups) and v == [1] * len(groups)
    small = sorted((c, g) for g, c in enumerate(groups) if c)[:3]
    assert gts == want_gts(lib, cid, fp, it, groups, oracle_for=[g for _, g in small])
    assert gts == identity(fp) * len(groups)
    # the coefficients belong to the item's index, not to the grouping: another grouping of the same items, same verdict
    rc2, v2, gts2 = run_combined(lib, cid, fp, it, [n - 100, 100])
    assert rc2 == 2 and v2 == [1, 1] and gts2 == identity(fp) * 2


@pytest.mark.parametrize("n", [1, 6, 7, 61, 200])
def test_one_group(gpu_lib, curve, n):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    it = items(lib, cid, fp, n, 1910 + n + cid)
    rc, v, gt = run_combined(lib, cid, fp, it, None)
    assert rc == 1 and v == [1]
    assert gt == want_gts(lib, cid, fp, it, None, oracle_for=[0] if n <= 7 else [])
    assert gt == identity(fp)
    assert run_combined(lib, cid, fp, it, [n])[1:] == ([1], gt)          # an explicit single group: the same path
    it["r"][n // 2] += 1
    rc, v, gt = run_combined(lib, cid, fp, it, None)
    assert rc == 0 and v == [0]
    assert gt == want_gts(lib, cid, fp, it, None) != identity(fp)
    assert run_combined(lib, cid, fp, it, [n])[1:] == ([0], gt)


def test_rejection_and_isolation(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G2B = 4 * fp
    groups = [7, 1, 6, 0, 12, 5, 61, 3, 2, 8, 4, 9]
    n = sum(groups)
    it = items(lib, cid, fp, n, 1920 + cid)
    start = lambda g: sum(groups[:g])
    it["m"][start(2) + 3] ^= 1 << 9                          # group 2: a changed m
    it["sig"][start(6) + 60] = it["sig"][start(6)]           # group 6: another signer's sigma
    k = it["key"][start(9) + 1]
    it["key"][start(9) + 1] = k[G2B:] + k[:G2B]              # group 9: U and V swapped
    rc, v, gts = run_combined(lib, cid, fp, it, groups)
    assert v == [0 if g in (2, 6, 9) else 1 for g in range(12)] and rc == 9
    assert gts == want_gts(lib, cid, fp, it, groups)
    singles = per_item(lib, cid, fp, it)
    assert v == [int(all(singles[start(g):start(g) + groups[g]])) for g in range(12)]


def test_the_cancellation_pair(gpu_lib, curve):
    """sigma + D and sigma - D under one Q: the product with unit coefficients is e(g1, g2)^2, what two valid items give"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G1B = 2 * fp
    rnd = random.Random(1930 + cid)
    q = tb.order_of(cid)
    x, y, m, r = rnd.randrange(1, q), rnd.randrange(1, q), rnd.randrange(0, q), rnd.randrange(1, q)
    u, v_ = tb.scale_gen(lib, cid, fp, 2, [x, y])
    sig, D = tb.scale_gen(lib, cid, fp, 1, [tb.sign_exp(cid, x, y, m, r), rnd.randrange(1, q)])
    nD = out(G1B)
    assert lib.bgls_scale_points(cid, 1, B(D), B(bytes(31) + b"\x01"), B(b"\x01"), 1, nD) == 0
    up, down = out(G1B), out(G1B)
    assert lib.bgls_point_add(cid, 1, B(sig), B(D), up) == 0
    assert lib.bgls_point_add(cid, 1, B(sig), nD, down) == 0
    good = {"sig": [sig, sig], "r": [r, r], "key": [u + v_] * 2, "m": [m, m]}
    bad = dict(good, sig=[bytes(up), bytes(down)])
    g1, g2 = gen(lib, cid, fp, 1), gen(lib, cid, fp, 2)
    Q = stepwise_q(lib, cid, fp, u + v_, r, m)
    unit, ref2 = out(12 * fp), out(12 * fp)
    assert lib.bgls_pairing_product(cid, B(bytes(up) + bytes(down)), B(Q + Q), 2, unit) == 0
    assert lib.bgls_pairing_product(cid, B(g1 + g1), B(g2 + g2), 2, ref2) == 0
    assert bytes(unit) == bytes(ref2)                        # the gap: a check with every coefficient 1 accepts the pair
    assert per_item(lib, cid, fp, good) == [1, 1] and per_item(lib, cid, fp, bad) == [0, 0]
    assert run_combined(lib, cid, fp, good, None)[:2] == (1, [1])
    for seed in (SEED, bytes(32), b"\xa5" * 32):
        assert run_combined(lib, cid, fp, bad, None, seed=seed)[:2] == (0, [0])
        assert run_combined(lib, cid, fp, bad, [2], seed=seed)[:2] == (0, [0])


def test_edge_items(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G1B, G2B = 2 * fp, 4 * fp
    groups = [3, 3, 3, 3, 3, 0, 2]
    it = items(lib, cid, fp, sum(groups), 1940 + cid)
    it["sig"][1] = bytes(G1B)                                # group 0: sigma at infinity
    k, r4, m4 = it["key"][4], it["r"][4], it["m"][4]         # group 1: U = -(m g2 + r V), Q at infinity
    part = coracle.aggregate_points(cid, 2, coracle.scale_point(cid, 2, gen(lib, cid, fp, 2), m4) + coracle.scale_point(cid, 2, k[G2B:], r4), 2)
    it["key"][4] = coracle.scale_point(cid, 2, part, -1) + k[G2B:]
    assert stepwise_q(lib, cid, fp, it["key"][4], r4, m4) == bytes(G2B)
    it["r"][6] = 0                                           # group 2: r = 0
    it["m"][11] = 0                                          # group 3: m = 0
    it["r"][12] = (1 << 256) - 1                             # group 4: the largest magnitude, unreduced
    rc, v, gts = run_combined(lib, cid, fp, it, groups)
    assert (rc, v) == (2, [0, 0, 0, 0, 0, 1, 1])
    assert gts == want_gts(lib, cid, fp, it, groups)
    assert gts[5 * 12 * fp:6 * 12 * fp] == identity(fp)
    assert [int(all(c)) for c in zip(*[iter(per_item(lib, cid, fp, it)[:15])] * 3)] == [0] * 5
    # the same items as one group, and a call of one group that holds nothing but the item with sigma at infinity
    rc, v, gt = run_combined(lib, cid, fp, it, None)
    assert (rc, v) == (0, [0]) and gt == want_gts(lib, cid, fp, it, None)
    lone = {k_: [x[1]] for k_, x in it.items()}
    rc, v, gt = run_combined(lib, cid, fp, lone, None)
    assert (rc, v) == (0, [0]) and gt == want_gts(lib, cid, fp, lone, None)


def test_whole_call_errors(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G2B = 4 * fp
    groups = [64, 66, 70]
    it = items(lib, cid, fp, 200, 1910 + 200 + cid)
    assert run_combined(lib, cid, fp, it, groups, want_gt=False)[:2] == (3, [1, 1, 1])
    for g in (groups, None):
        bad = {k: list(x) for k, x in it.items()}
        raw = bytearray(bad["sig"][130])
        raw[-1] ^= 1                                         # an off-curve sigma
        bad["sig"][130] = bytes(raw)
        assert run_combined(lib, cid, fp, bad, g, want_gt=False)[0] == ERR_ENCODING
        bad = {k: list(x) for k, x in it.items()}
        raw = bytearray(bad["key"][199])
        raw[:fp] = b"\xff" * fp                              # a non-canonical U, far from item 0
        bad["key"][199] = bytes(raw)
        assert run_combined(lib, cid, fp, bad, g, want_gt=False)[0] == ERR_ENCODING
        bad = {k: list(x) for k, x in it.items()}
        raw = bytearray(bad["key"][77])
        raw[2 * G2B - 1] ^= 1                                # an off-curve V
        bad["key"][77] = bytes(raw)
        assert run_combined(lib, cid, fp, bad, g, want_gt=False)[0] == ERR_ENCODING
        rc, v, gts = run_combined(lib, cid, fp, it, g)       # the next valid call is correct
        assert rc == len(v) and set(v) == {1} and gts == identity(fp) * len(v)


def launches(lib, stage):
    t, cnt = ctypes.c_double(), ctypes.c_ulonglong()
    assert lib.bgls_profile_get(stage.encode(), ctypes.byref(t), ctypes.byref(cnt)) == 0
    return cnt.value


def test_device_form_streams_modes_and_profile_scopes(gpu_lib, curve):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    groups = [64, 0, 61, 25]
    it = items(lib, cid, fp, 150, 1960 + cid)
    it["m"][70] += 1
    dev = torch.device("cuda:0")
    d = [torch.tensor(list(bytes(x)), dtype=torch.uint8, device=dev) for x in packed(it)]
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()

    def run_dev(g, stream=None):
        ng = 1 if g is None else len(g)
        v, gt = out(ng), out(ng * 12 * fp)
        rc = lib.bgls_bb_verify_batch_combined_dev(cid, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), 150,
                                                   None if g is None else offs(g), ng, B(SEED), v, gt, stream)
        return rc, list(v)[:ng], bytes(gt)[:ng * 12 * fp]

    results = []
    try:
        for mode in (0, 1):
            assert lib.bgls_set_throughput_mode(mode) == 0
            results.append((run_combined(lib, cid, fp, it, groups), run_dev(groups), run_dev(groups, side.cuda_stream), run_combined(lib, cid, fp, it, None),
                            run_dev(None), run_dev(None, side.cuda_stream)))
    finally:
        lib.bgls_set_throughput_mode(0)
    host, devr, devs, host1, dev1, devs1 = results[0]
    assert host[:2] == (3, [1, 1, 0, 1]) and host1[:2] == (0, [0])
    assert host[2] == want_gts(lib, cid, fp, it, groups) and host1[2] == want_gts(lib, cid, fp, it, None)
    assert devr == host and devs == host and dev1 == host1 and devs1 == host1
    assert results[1] == results[0]
    want = {"bb_keys": 1, "rlc": 1, "miller": 1, "final_exp": 1, "h2c": 0, "sum_points": 0, "dup_check": 0}
    for g, call in ((groups, run_dev), (None, run_dev), (groups, lambda g: run_combined(lib, cid, fp, it, g, want_gt=False))):
        try:
            assert lib.bgls_profile_enable(1) == 0
            assert call(g)[0] == (3 if g else 0)
            assert {s: launches(lib, s) for s in want} == want, g
            assert launches(lib, "epilogue") == (1 if g else 0) and launches(lib, "scatter") == (1 if g else 0)
            # the call has no stage of its own: its work shows under bb_keys and rlc
            t, cnt = ctypes.c_double(), ctypes.c_ulonglong()
            for name in (b"bb_rlc", b"bb_combined", b"bb_rlc_sums"):
                assert lib.bgls_profile_get(name, ctypes.byref(t), ctypes.byref(cnt)) != 0
        finally:
            lib.bgls_profile_enable(0)


def _mirror_items(cv, it):
    from bgls_amd import bbsigs
    from bgls_amd.curves import Point, G1, G2
    G2B = len(it["key"][0]) // 2
    sigs = [bbsigs.Signature(Point(cv, G1, s), r) for s, r in zip(it["sig"], it["r"])]
    pks = [bbsigs.Pubkey(Point(cv, G2, k[:G2B]), Point(cv, G2, k[G2B:])) for k in it["key"]]
    return sigs, pks, list(it["m"])


def test_4096_items_and_the_located_fallback(gpu_lib, curve, monkeypatch):
    from bgls_amd import Altbn128, Bls12, bbsigs
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Altbn128 if cid == 0 else Bls12
    n = 1 << 12
    it = items(lib, cid, fp, n, 1970 + cid)
    assert run_combined(lib, cid, fp, it, None, want_gt=False)[:2] == (1, [1])
    assert run_combined(lib, cid, fp, it, [64] * 64, want_gt=False)[:2] == (64, [1] * 64)
    it["r"][1000] += 1
    it["sig"][3001] = it["sig"][3000]
    assert run_combined(lib, cid, fp, it, None, want_gt=False)[:2] == (0, [0])
    assert run_combined(lib, cid, fp, it, [64] * 64, want_gt=False)[1] == [int(g not in (1000 // 64, 3001 // 64)) for g in range(64)]
    sigs, pks, msgs = _mirror_items(cv, it)
    seen, plain = [], bbsigs.VerifyBatch
    monkeypatch.setattr(bbsigs, "VerifyBatch", lambda c, s, k, m: seen.append(len(s)) or plain(c, s, k, m))
    got = bbsigs.VerifyBatchLocated(cv, sigs, pks, msgs)
    assert got == [b not in (1000, 3001) for b in range(n)]
    assert seen == [128]                                     # ONE per-item call over the items of the two rejected groups, not over 4096


def test_python_mirrors(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bbsigs
    cv, other = (Altbn128, Bls12) if curve["id"] == 0 else (Bls12, Altbn128)
    rnd = random.Random(1980 + curve["id"])
    sigs, pks, msgs, hsigs, hmsgs = [], [], [], [], []
    for i in range(7):
        sk, pk = bbsigs.KeyGen(cv)
        m = rnd.randrange(0, 1 << 300) if i % 3 else -rnd.randrange(1, 1 << 200)
        hm = [b"", b"\x00", bytes(range(128)), bytes(range(129))][i % 4]
        sigs.append(bbsigs.Sign(cv, sk, m))
        hsigs.append(bbsigs.SignHashed(cv, sk, hm))
        pks.append(pk)
        msgs.append(m)
        hmsgs.append(hm)
    assert bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs) == [True]
    assert bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs, group=3, seed=SEED) == [True, True, True]
    assert bbsigs.VerifyBatchLocated(cv, sigs, pks, msgs, group=2) == [True] * 7
    assert bbsigs.VerifyBatchCombined(cv, [], [], []) == []
    assert bbsigs.VerifyHashedBatchCombined(cv, hsigs, pks, hmsgs, group=4) == [True, True]
    assert bbsigs.VerifyHashedBatchLocated(cv, hsigs, pks, hmsgs) == [True] * 7
    msgs[4] += 1
    hmsgs[5] += b"x"
    assert bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs) == [False]
    assert bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs, group=3) == [True, False, True]
    assert bbsigs.VerifyBatchLocated(cv, sigs, pks, msgs, group=3) == bbsigs.VerifyBatch(cv, sigs, pks, msgs) == [b != 4 for b in range(7)]
    assert bbsigs.VerifyHashedBatchLocated(cv, hsigs, pks, hmsgs, group=2) == bbsigs.VerifyHashedBatch(cv, hsigs, pks, hmsgs) == [b != 5 for b in range(7)]
    with pytest.raises(ValueError):
        bbsigs.VerifyBatchCombined(cv, sigs, pks, msgs, seed=b"short")
    osk, opk = bbsigs.KeyGen(other)
    with pytest.raises(ValueError):
        bbsigs.VerifyBatchCombined(cv, sigs[:6] + [bbsigs.Sign(other, osk, 4)], pks, msgs)      # a foreign-curve point
    with pytest.raises(ValueError):
        bbsigs.VerifyBatchCombined(cv, sigs, pks[:6] + [bbsigs.Pubkey(None, pks[6].V)], msgs)   # a nil point
    with pytest.raises(ValueError):
        bbsigs.VerifyBatchCombined(cv, sigs, pks[:6], msgs)
