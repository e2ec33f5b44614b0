"""GPU tier: n independent Boneh-Boyen verifications (bbsigs.Verify, bbsigs/bbsigs.go:68-73) in one set of launches
(bgls_bb_verify_batch / _dev): valid signatures built with the C oracle, mixed batches checked item by item against the oracle's
pairing, GT bytes against bgls_pair of the stepwise per-point Q = m g2 + U + r V, the exceptional cases (zero and oversized scalars,
points at infinity, Q at infinity, an off-subgroup V), batch sizes around k_miller_sets' 30 sets per block and k_bb_keys' 64-lane
block, 2^16 items, whole-call errors, the device form, the profile scopes and the Python mirror (TestSignatureConsistency)."""
import ctypes
import json
import os
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ENCODING = -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


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


def sign_exp(cid, x, y, m, r):
    q = order_of(cid)
    return pow((x + m + y * r) % q, -1, q)


def make_items(lib, cid, fp, n, seed):
    """n valid (sigma, r, U || V, m) items; keys and signatures from the GPU's fixed-base generator multiples"""
    rnd = random.Random(seed)
    q = order_of(cid)
    xs = [rnd.randrange(1, q) for _ in range(n)]
    ys = [rnd.randrange(1, q) for _ in range(n)]
    ms = [rnd.randrange(0, 1 << 256) for _ in range(n)]
    rs = [rnd.randrange(1, q) for _ in range(n)]
    us, vs = scale_gen(lib, cid, fp, 2, xs), scale_gen(lib, cid, fp, 2, ys)
    sig = scale_gen(lib, cid, fp, 1, [sign_exp(cid, x, y, m, r) for x, y, m, r in zip(xs, ys, ms, rs)])
    return {"sig": sig, "r": rs, "key": [u + v for u, v in zip(us, vs)], "m": ms}


def run(lib, cid, fp, it, want_gt=True):
    n = len(it["sig"])
    v = out(n)
    gt = out(n * 12 * fp) if want_gt else None
    rc = lib.bgls_bb_verify_batch(cid, B(b"".join(it["sig"])), B(b"".join(r.to_bytes(32, "big") for r in it["r"])), B(b"".join(it["key"])),
                                  B(b"".join(m.to_bytes(32, "big") for m in it["m"])), n, v, gt)
    return rc, list(v)[:n], ([bytes(gt)[b * 12 * fp:(b + 1) * 12 * fp] for b in range(n)] if want_gt else None)


def stepwise_q(lib, cid, fp, key, r, m):
    """Q = m g2 + U + r V with the per-point calls (what a Go caller of bbsigs.Verify does today)"""
    G2B = 4 * fp
    mg2 = out(G2B)
    assert lib.bgls_scale_generator(cid, 2, B(m.to_bytes(32, "big")), 1, mg2) == 0
    rv = out(G2B)
    assert lib.bgls_scale_points(cid, 2, B(key[G2B:]), B(r.to_bytes(32, "big")), B(b"\0"), 1, rv) == 0
    t, q = out(G2B), out(G2B)
    assert lib.bgls_point_add(cid, 2, mg2, B(key[:G2B]), t) == 0
    assert lib.bgls_point_add(cid, 2, t, rv, q) == 0
    return bytes(q)


def pair(lib, cid, fp, g1, g2):
    o = out(12 * fp)
    assert lib.bgls_pair(cid, B(g1), B(g2), o) == 0
    return bytes(o)


def oracle_verdict(cid, fp, g1, g2, sig, key, r, m):
    """independent per-item check on the C oracle: e(sigma, m g2 + U + r V) == e(g1, g2)"""
    G2B = 4 * fp
    parts = coracle.scale_point(cid, 2, g2, m) + key[:G2B] + coracle.scale_point(cid, 2, key[G2B:], r)
    q = coracle.aggregate_points(cid, 2, parts, 3)
    return int(coracle.final_exp(cid, coracle.miller(cid, sig, q)) == coracle.final_exp(cid, coracle.miller(cid, g1, g2)))


def check_items(lib, cid, fp, it, verdicts, gts, oracle_every=1):
    g1, g2 = gen(lib, cid, fp, 1), gen(lib, cid, fp, 2)
    gt_ref = pair(lib, cid, fp, g1, g2)
    for b in range(len(it["sig"])):
        q = stepwise_q(lib, cid, fp, it["key"][b], it["r"][b], it["m"][b])
        want_gt = pair(lib, cid, fp, it["sig"][b], q)
        assert gts[b] == want_gt, b
        assert verdicts[b] == int(want_gt == gt_ref), b
        if oracle_every and b % oracle_every == 0:
            assert verdicts[b] == oracle_verdict(cid, fp, g1, g2, it["sig"][b], it["key"][b], it["r"][b], it["m"][b]), b


def test_valid_signatures_from_the_oracle(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(5 + cid)
    q = order_of(cid)
    g1, g2 = gen(lib, cid, fp, 1), gen(lib, cid, fp, 2)
    it = {"sig": [], "r": [], "key": [], "m": []}
    for _ in range(12):
        x, y, m, r = rnd.randrange(1, q), rnd.randrange(1, q), rnd.randrange(0, q), rnd.randrange(1, 1 << 256)
        it["key"].append(coracle.scale_point(cid, 2, g2, x) + coracle.scale_point(cid, 2, g2, y))
        it["sig"].append(coracle.scale_point(cid, 1, g1, sign_exp(cid, x, y, m, r)))
        it["r"].append(r)
        it["m"].append(m)
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc == 12 and verdicts == [1] * 12
    gt_ref = pair(lib, cid, fp, g1, g2)
    assert all(g == gt_ref for g in gts)


def test_mixed_batch_per_item_verdicts(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G2B = 4 * fp
    n = 40
    it = make_items(lib, cid, fp, n + 1, 11 + cid)
    spare_key = it["key"][n]
    for k in it:
        it[k] = it[k][:n]
    rnd = random.Random(13 + cid)
    bad = rnd.sample(range(n), 10)
    for j, b in enumerate(bad):
        kind = j % 5
        if kind == 0:
            it["r"][b] += 1                                # a changed r
        elif kind == 1:
            it["m"][b] ^= 1 << 7                           # a changed m
        elif kind == 2:
            it["sig"][b] = it["sig"][(b + 1) % n]          # another signer's sigma
        elif kind == 3:
            k = it["key"][b]
            it["key"][b] = k[G2B:] + k[:G2B]               # U and V swapped
        else:
            it["key"][b] = spare_key                       # another signer's key
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc == n - len(bad) and rc == sum(verdicts)
    assert [b for b in range(n) if not verdicts[b]] == sorted(bad)
    check_items(lib, cid, fp, it, verdicts, gts, oracle_every=3)


def _fixture_v(curve):
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "subgroup_%s.json" % curve["name"])))
    return [bytes.fromhex(p["pt"]) for p in fix["points"] if p.get("on_twist") and not p.get("in_subgroup") and not p.get("miller_degenerates")]


def test_edge_cases_match_the_stepwise_path(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G1B, G2B = 2 * fp, 4 * fp
    q = order_of(cid)
    it = make_items(lib, cid, fp, 12, 17 + cid)
    inf2 = bytes(G2B)
    it["r"][0] = 0                                         # r = 0
    it["m"][1] = 0                                         # m = 0
    it["r"][2] = q                                         # r = order: r V = infinity
    it["r"][3] = (1 << 256) - 1                            # the largest magnitude, unreduced
    it["key"][4] = inf2 + it["key"][4][G2B:]               # U at infinity
    it["key"][5] = it["key"][5][:G2B] + inf2               # V at infinity
    it["sig"][6] = bytes(G1B)                              # sigma at infinity
    # U = -(m g2 + r V): Q at infinity
    k7, r7, m7 = it["key"][7], it["r"][7], it["m"][7]
    part = coracle.aggregate_points(cid, 2, coracle.scale_point(cid, 2, gen(lib, cid, fp, 2), m7) + coracle.scale_point(cid, 2, k7[G2B:], r7), 2)
    it["key"][7] = coracle.scale_point(cid, 2, part, -1) + k7[G2B:]
    assert stepwise_q(lib, cid, fp, it["key"][7], r7, m7) == inf2
    # an off-subgroup point as V (exactness of r V off the subgroup); also r = 2^256 - 1 on it
    offs = _fixture_v(curve)
    assert offs
    it["key"][8] = it["key"][8][:G2B] + offs[0]
    it["key"][9] = it["key"][9][:G2B] + offs[-1]
    it["r"][9] = (1 << 256) - 1
    it["r"][10] = q + 5                                    # above the order: used as given
    it["m"][11] = (1 << 256) - 1
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc >= 0, rc
    assert verdicts[:8] == [0, 0, 0, 0, 0, 0, 0, 0] and verdicts[8] == 0 and verdicts[9] == 0
    check_items(lib, cid, fp, it, verdicts, gts, oracle_every=0)
    one = out(12 * fp)
    assert lib.bgls_gt_identity(cid, one) == 0
    assert gts[6] == bytes(one) and gts[7] == bytes(one)  # e(inf, Q) = e(sigma, inf) = 1


@pytest.mark.parametrize("n", [1, 29, 30, 31, 61, 1000])
def test_batch_sizes(gpu_lib, curve, n):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    it = make_items(lib, cid, fp, n, 100 + n + cid)
    if n > 1:
        it["r"][n - 1] += 1
        it["m"][n // 2] += 1
    rc, verdicts, gts = run(lib, cid, fp, it)
    want = [1] * n
    if n > 1:
        want[n - 1] = 0
        want[n // 2] = 0
    assert verdicts == want and rc == sum(want)
    check_items(lib, cid, fp, it, verdicts, gts, oracle_every=97)


def test_2_16_items(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 1 << 16
    it = make_items(lib, cid, fp, n, 23 + cid)
    bad = [0, 1, 29, 30, 4095, 4096, 40000, n - 1]
    for j, b in enumerate(bad):
        if j % 2:
            it["r"][b] += 1
        else:
            it["sig"][b] = it["sig"][(b + 7) % n]
    rc, verdicts, _ = run(lib, cid, fp, it, want_gt=False)
    assert rc == n - len(bad)
    assert [b for b in range(n) if not verdicts[b]] == bad


def test_whole_call_errors_and_device_form(gpu_lib, curve):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    G1B, G2B = 2 * fp, 4 * fp
    it = make_items(lib, cid, fp, 70, 31 + cid)
    it["r"][3] += 1
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc == 69
    for slot in ("sig", "U", "V"):
        for kind in ("offcurve", "noncanon"):
            bad = dict((k, list(v)) for k, v in it.items())
            b = 45
            if slot == "sig":
                raw = bytearray(bad["sig"][b])
                if kind == "offcurve":
                    raw[-1] ^= 1
                else:
                    raw[:fp] = b"\xff" * fp                 # x not below the field modulus
                bad["sig"][b] = bytes(raw)
            else:
                raw = bytearray(bad["key"][b])
                off = 0 if slot == "U" else G2B
                if kind == "offcurve":
                    raw[off + G2B - 1] ^= 1
                else:
                    raw[off:off + fp] = b"\xff" * fp
                bad["key"][b] = bytes(raw)
            assert run(lib, cid, fp, bad, want_gt=False)[0] == ERR_ENCODING, (slot, kind)
    # the device form: same verdicts and GT bytes
    dev = torch.device("cuda")
    n = len(it["sig"])
    d = [torch.tensor(list(x), dtype=torch.uint8, device=dev) for x in (b"".join(it["sig"]), b"".join(r.to_bytes(32, "big") for r in it["r"]),
                                                                        b"".join(it["key"]), b"".join(m.to_bytes(32, "big") for m in it["m"]))]
    torch.cuda.synchronize()
    v2, gt2 = out(n), out(n * 12 * fp)
    assert lib.bgls_bb_verify_batch_dev(cid, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, v2, gt2, None) == 69
    assert list(v2)[:n] == verdicts
    assert [bytes(gt2)[b * 12 * fp:(b + 1) * 12 * fp] for b in range(n)] == gts


def test_profile_scopes(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    it = make_items(lib, cid, fp, 50, 37 + cid)

    def launches(stage):
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        assert lib.bgls_profile_get(stage.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0
        return cnt.value

    try:
        assert lib.bgls_profile_enable(1) == 0
        assert run(lib, cid, fp, it, want_gt=False)[0] == 50
        want = {"bb_keys": 1, "miller": 1, "final_exp": 1, "epilogue": 1 if cid == 1 else 0, "h2c": 0, "sum_points": 0, "scatter": 0, "reduce": 0,
                "dup_check": 0}
        assert {s: launches(s) for s in want} == want
    finally:
        lib.bgls_profile_enable(0)


def test_python_mirror_signature_consistency(gpu_lib, curve):
    """the reference's TestSignatureConsistency: KeyGen / Sign / Verify and the hashed forms, then the batch forms"""
    from bgls_amd import Altbn128, Bls12, bbsigs
    cv = Altbn128 if curve["id"] == 0 else Bls12
    rnd = random.Random(41 + curve["id"])
    sigs, pks, msgs = [], [], []
    for i in range(10):
        sk, pk = bbsigs.KeyGen(cv)
        m = rnd.randrange(0, 1 << 300) if i % 3 else -rnd.randrange(1, 1 << 200)
        sig = bbsigs.Sign(cv, sk, m)
        assert bbsigs.Verify(cv, sig, pk, m)
        assert not bbsigs.Verify(cv, sig, pk, m + 1)
        hm = [b"", b"\x00", bytes(range(128)), bytes(range(129))][i % 4]
        hs = bbsigs.SignHashed(cv, sk, hm)
        assert bbsigs.VerifyHashed(cv, hs, pk, hm)
        assert not bbsigs.VerifyHashed(cv, hs, pk, hm + b"x")
        assert bbsigs.VerifyCustHash(cv, hs, pk, hm, bbsigs.blake2b256)
        sigs.append(sig)
        pks.append(pk)
        msgs.append(m)
    msgs2 = list(msgs)
    msgs2[4] += 1
    sigs2 = list(sigs)
    sigs2[7] = bbsigs.Signature(sigs[6].Sigma, sigs[7].R)
    want = [bbsigs.Verify(cv, s, k, m) for s, k, m in zip(sigs2, pks, msgs2)]
    assert want == [i not in (4, 7) for i in range(10)]
    assert bbsigs.VerifyBatch(cv, sigs2, pks, msgs2) == want
    sk, pk = bbsigs.KeyGen(cv)
    hms = [b"", b"a", bytes(128), bytes(129)]
    hsig = [bbsigs.SignHashed(cv, sk, m) for m in hms]
    assert bbsigs.VerifyHashedBatch(cv, hsig, [pk] * 4, hms) == [True] * 4
    assert bbsigs.VerifyHashedBatch(cv, hsig[::-1], [pk] * 4, hms) == [False] * 4
    # SignBatch over one scale_generator call; a foreign point is rejected on its own
    sb = bbsigs.SignBatch(cv, [sk] * 3, [1, 2, 3])
    assert bbsigs.VerifyBatch(cv, sb, [pk] * 3, [1, 2, 3]) == [True] * 3
    other = Bls12 if curve["id"] == 0 else Altbn128
    osk, opk = bbsigs.KeyGen(other)
    assert bbsigs.VerifyBatch(cv, sb + [bbsigs.Sign(other, osk, 4)], [pk] * 3 + [opk], [1, 2, 3, 4]) == [True, True, True, False]


def _ref_q(cid, key, r, m):
    """Q = m g2 + U + r V by the plain affine reference (tests/ec_ref.py), scalars unreduced"""
    from ec_ref import Curve
    cv = Curve(cid, 2)
    G2B = cv.size
    return cv.to_bytes(cv.add(cv.add(cv.mul(cv.gen, m), cv.from_bytes(key[:G2B])), cv.mul(cv.from_bytes(key[G2B:]), r)))


def test_every_fixture_point_as_v_at_its_order(gpu_lib, curve):
    """k_bb_keys' windowed chain (rx_g2mul.hpp) on EVERY on-twist fixture point outside the subgroup as V -- the small-order ones included,
    also the one whose own Miller loop degenerates: Q = m g2 + U + r V is not that point (asserted with the plain reference) -- under a
    random r, r = order(V), order(V) +- 1 and 2^256 - 1.  Q's bytes against the plain reference, GT bytes and verdicts against the
    stepwise path."""
    import point_cases as pc
    from ec_ref import Curve
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Curve(cid, 2)
    G2B = 4 * fp
    rnd = random.Random(71 + cid)
    pts = pc.fixture_points(cid, 2)
    assert any(o is not None and o < 64 for _, o, _ in pts) or cid == 0
    plan = []
    for pt, order, note in pts:
        rs = [rnd.getrandbits(256), (1 << 256) - 1]
        if order is not None:
            rs += [order, order - 1, order + 1]
        plan += [(pt, r) for r in rs]
    it = make_items(lib, cid, fp, len(plan), 73 + cid)
    for b, (pt, r) in enumerate(plan):
        it["key"][b] = it["key"][b][:G2B] + cv.to_bytes(pt)
        it["r"][b] = r
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc >= 0, rc
    for b, (pt, r) in enumerate(plan):
        want_q = _ref_q(cid, it["key"][b], r, it["m"][b])
        assert want_q != cv.to_bytes(pt) and want_q != bytes(G2B), b
        assert stepwise_q(lib, cid, fp, it["key"][b], r, it["m"][b]) == want_q, (b, hex(r))
    check_items(lib, cid, fp, it, verdicts, gts, oracle_every=0)
    assert verdicts == [0] * len(plan)


def test_fixed_base_chain_meets_its_own_table_entry(gpu_lib, curve):
    """k_bb_keys folds m g2 in with one mixed addition (jacx_madd) per non-zero byte of m against the table d 2^(8 j) g2.  With V at
    infinity or r = 0 the running point is U when byte j arrives: U = d 2^(8 j) g2 makes that addition a DOUBLING, U = -d 2^(8 j) g2
    makes the sum pass through infinity and go on with the higher bytes of m.  Q's bytes against the plain reference, GT bytes and
    verdicts against the stepwise path."""
    from ec_ref import Curve
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Curve(cid, 2)
    G2B = 4 * fp
    rnd = random.Random(79 + cid)
    spots = [(0, 1), (0, 255), (1, 7), (5, 128), (15, 200), (31, 1), (31, 255)]          # (byte position j of m, its value d)
    plan = []
    for j, d in spots:
        for neg in (False, True):
            for v_inf in (False, True):
                for higher in (False, True):
                    if higher and j == 31:
                        continue
                    m = d << (8 * j)                                       # only byte j below: the running point is still U there
                    if higher:
                        m |= rnd.getrandbits(8 * (31 - j)) << (8 * (j + 1)) | 1 << 255
                    plan.append((j, d, neg, v_inf, m))
    it = make_items(lib, cid, fp, len(plan), 83 + cid)
    for b, (j, d, neg, v_inf, m) in enumerate(plan):
        u = cv.mul(cv.gen, d << (8 * j))
        it["key"][b] = cv.to_bytes(cv.neg(u) if neg else u) + (bytes(G2B) if v_inf else it["key"][b][G2B:])
        it["r"][b] = it["r"][b] if v_inf else 0
        it["m"][b] = m
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc >= 0, rc
    for b, (j, d, neg, v_inf, m) in enumerate(plan):
        want_q = _ref_q(cid, it["key"][b], it["r"][b], m)
        if neg and m == d << (8 * j):
            assert want_q == bytes(G2B)
        assert stepwise_q(lib, cid, fp, it["key"][b], it["r"][b], m) == want_q, plan[b]
    check_items(lib, cid, fp, it, verdicts, gts, oracle_every=0)


def test_u_equals_r_v_when_the_chain_ends_on_a_doubling(gpu_lib, curve):
    """r = 16 c ends the windowed chain on four doublings (a zero last digit), so r V reaches the mixed addition of U straight from
    jacx_dbl, whose Y is not reduced; with U = r V that addition must DOUBLE.  Q = 2 U (m = 0) and Q = 2 U + m g2 against the plain
    reference; GT bytes and verdicts against the stepwise path."""
    from ec_ref import Curve
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Curve(cid, 2)
    G2B = 4 * fp
    rnd = random.Random(89 + cid)
    n = 48
    it = make_items(lib, cid, fp, n, 97 + cid)
    for b in range(n):
        v = cv.from_bytes(it["key"][b][G2B:])
        r = 16 * rnd.choice([1, 2, 3, 16, 255, rnd.getrandbits(60), rnd.getrandbits(250)])
        u = cv.mul(v, r)
        it["key"][b] = cv.to_bytes(u if b % 4 else cv.neg(u)) + it["key"][b][G2B:]
        it["r"][b] = r
        it["m"][b] = 0 if b % 3 else rnd.getrandbits(256)
    rc, verdicts, gts = run(lib, cid, fp, it)
    assert rc >= 0, rc
    for b in range(n):
        want_q = _ref_q(cid, it["key"][b], it["r"][b], it["m"][b])
        assert stepwise_q(lib, cid, fp, it["key"][b], it["r"][b], it["m"][b]) == want_q, b
    check_items(lib, cid, fp, it, verdicts, gts, oracle_every=0)
