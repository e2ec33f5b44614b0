"""GPU tier: many multi-signatures under one combined check per group (bgls_verify_multi_sets_combined / _dev, bgls_rlc_coefficients).
The coefficients against the oracle's BLAKE2Xb; every group's GT element byte for byte against bgls_pairing_product over pairs built
with the existing point calls (and the C oracle's product for the smallest groups); ragged sets and group sizes around the six-pairing
padding, the 60-pairing block and the 64-lane edge of k_rlc_pair; the single-group path; rejection and isolation; the cancellation pair
that bgls_verify_multi_batch accepts; infinity; whole-call errors; the device form, throughput modes and profile scopes; 2^12 one-key
sets with the located fallback; the Python mirrors."""
import ctypes
import random

import pytest

import test_gpu_multi_sets as ms
from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2
B, out, offs = ms.B, ms.out, ms.offs
SET_SIZES = [0, 1, 2, 127, 128, 129]
GROUP_SIZES = [0, 1, 5, 6, 7, 59, 60, 61, 63, 64, 65]
SEED = bytes(range(32))


def coefficients(lib, seed, n):
    r = out(16 * n)
    assert lib.bgls_rlc_coefficients(B(seed), n, r) == 0
    return bytes(r)[:16 * n]


def want_coefficients(seed, n):
    raw = bytearray(coracle.blake2xb(b"bgls-rlc-v1" + seed + n.to_bytes(8, "little"), 16 * n))
    for b in range(n):
        raw[16 * b + 15] |= 1
    return bytes(raw)


def run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups, seed=SEED, want_gt=True):
    """groups: the list of group sizes, or None for group_off = NULL"""
    n, ng = len(sizes), (1 if groups is None else len(groups))
    v = out(ng)
    gt = out(ng * 12 * fp) if want_gt else None
    rc = lib.bgls_verify_multi_sets_combined(cid, B(b"".join(sigs)), B(keys), offs(sizes), n, B(b"".join(msgs)), offs([len(m) for m in msgs]),
                                             None if groups is None else offs(groups), ng, B(seed), v, gt)
    return rc, list(v)[:ng], (bytes(gt)[:ng * 12 * fp] if want_gt else None)


def identity(fp):
    return bytes(12 * fp - 1) + b"\x01"


def group_pairs(lib, cid, fp, sizes, keys, msgs, sigs, seed):
    """per set b: r_b H(m_b), apk_b and -r_b sigma_b as wire bytes, from the existing calls"""
    n = len(sizes)
    r = coefficients(lib, seed, n)
    sc = B(b"".join(bytes(16) + r[16 * b:16 * b + 16] for b in range(n)))
    hs, rh, rs, apks = out(n * 2 * fp), out(n * 2 * fp), out(n * 2 * fp), out(n * 4 * fp)
    assert lib.bgls_hash_to_g1(cid, B(b"".join(msgs)), offs([len(m) for m in msgs]), n, hs) == 0
    assert lib.bgls_scale_points(cid, 1, hs, sc, None, n, rh) == 0
    assert lib.bgls_scale_points(cid, 1, B(b"".join(sigs)), sc, B(b"\x01" * n), n, rs) == 0
    assert lib.bgls_aggregate_sets(cid, 2, B(keys), offs(sizes), n, apks) == 0
    return bytes(rh), bytes(apks), bytes(rs)


def want_gts(lib, cid, fp, sizes, keys, msgs, sigs, groups, seed, oracle_for=()):
    n = len(sizes)
    groups = [n] if groups is None else groups
    rh, apks, rs = group_pairs(lib, cid, fp, sizes, keys, msgs, sigs, seed)
    nsig = out(len(groups) * 2 * fp)
    assert lib.bgls_aggregate_sets(cid, 1, B(rs), offs(groups), len(groups), nsig) == 0        # -sum_b r_b sigma_b per group
    g2 = out(4 * fp)
    assert lib.bgls_generator(cid, 2, g2) == 0
    res, at = [], 0
    for g, c in enumerate(groups):
        if c == 0:
            res.append(identity(fp))
            continue
        g1s = rh[at * 2 * fp:(at + c) * 2 * fp] + bytes(nsig)[g * 2 * fp:(g + 1) * 2 * fp]
        g2s = apks[at * 4 * fp:(at + c) * 4 * fp] + bytes(g2)
        gt = out(12 * fp)
        assert lib.bgls_pairing_product(cid, B(g1s), B(g2s), c + 1, gt) == 0
        res.append(bytes(gt))
        if g in oracle_for:
            assert coracle.pairing_product(cid, g1s, g2s, c + 1, threads=8) == bytes(gt), g
        at += c
    return b"".join(res)


def test_coefficients(gpu_lib):
    lib = gpu_lib
    for n in (1, 4, 5, 1000):
        got = coefficients(lib, SEED, n)
        assert got == want_coefficients(SEED, n), n
        assert all(got[16 * b + 15] & 1 for b in range(n))
        assert coefficients(lib, SEED, n) == got
        assert coefficients(lib, bytes(31) + b"\x01", n) != got


def test_ragged_sets_and_groups(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(900 + cid)
    groups = list(GROUP_SIZES)
    rnd.shuffle(groups)
    n = sum(groups)                                          # 391 sets
    sizes = [rnd.choice(SET_SIZES) if b % 5 == 0 else rnd.choice(SET_SIZES[:3]) for b in range(n)]
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 901 + cid)
    sigs = [bytes(2 * fp) if c == 0 else s for c, s in zip(sizes, sigs)]     # an empty set signs with the point at infinity
    rc, v, gts = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups)
    assert rc == len(groups) and v == [1] * len(groups)
    small = sorted((c, g) for g, c in enumerate(groups) if c)[:3]
    assert gts == want_gts(lib, cid, fp, sizes, keys, msgs, sigs, groups, SEED, oracle_for=[g for _, g in small])
    assert gts[groups.index(0) * 12 * fp:][:12 * fp] == identity(fp)
    assert set(gts[g * 12 * fp:(g + 1) * 12 * fp] for g in range(len(groups))) == {identity(fp)}
    # the coefficients belong to the set's index, not to the grouping: another grouping of the same sets, same verdict
    rc2, v2, _ = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, [n - 100, 100], want_gt=False)
    assert rc2 == 2 and v2 == [1, 1]


@pytest.mark.parametrize("n", [1, 6, 7, 61, 200])
def test_one_group(gpu_lib, curve, n):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(n)
    sizes = [rnd.choice(SET_SIZES[1:3]) for _ in range(n)]
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 910 + n + cid)
    rc, v, gt = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None)
    assert rc == 1 and v == [1]
    assert gt == want_gts(lib, cid, fp, sizes, keys, msgs, sigs, None, SEED, oracle_for=[0] if n <= 7 else [])
    assert gt == identity(fp)
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, [n])[1:] == ([1], gt)           # an explicit single group: the same path
    msgs[n // 2] += b"!"
    rc, v, gt = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None)
    assert rc == 0 and v == [0]
    assert gt == want_gts(lib, cid, fp, sizes, keys, msgs, sigs, None, SEED) != identity(fp)


def test_rejection_and_isolation(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    groups = [7, 1, 6, 0, 12, 5, 61, 3, 2, 8, 4, 9]
    n = sum(groups)
    sizes = [1 + b % 3 for b in range(n)]
    keys, msgs, sigs, spare = ms.make_sets(lib, cid, fp, sizes, 920 + cid)
    keys = bytearray(keys)
    start = lambda g: sum(groups[:g])
    msgs[start(2) + 3] += b"x"                               # group 2: a wrong message
    sigs[start(6) + 60] = sigs[start(6)]                     # group 6: a wrong signature
    k = sum(sizes[:start(9) + 1])
    keys[k * 4 * fp:(k + 1) * 4 * fp] = spare                # group 9: a key swapped for a spare
    keys = bytes(keys)
    rc, v, gts = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups)
    assert v == [0 if g in (2, 6, 9) else 1 for g in range(12)] and rc == 9
    assert gts == want_gts(lib, cid, fp, sizes, keys, msgs, sigs, groups, SEED)
    singles, at = [], 0
    for b, c in enumerate(sizes):
        singles.append(ms.single(lib, cid, sigs[b], keys[at * 4 * fp:(at + c) * 4 * fp], c, msgs[b]))
        at += c
    assert v == [int(all(singles[start(g):start(g) + groups[g]])) for g in range(12)]


def test_the_cancellation_pair(gpu_lib, curve):
    """sigma_1 + D and sigma_2 - D: the sum of the signatures is unchanged, so the r_b = 1 form accepts the batch"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [2, 3]
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 930 + cid)
    D = out(2 * 2 * fp)
    assert lib.bgls_hash_to_g1(cid, B(b"shift" * 2), offs([5, 5]), 2, D) == 0
    shift = out(2 * 2 * fp)
    assert lib.bgls_scale_points(cid, 1, D, B(bytes(31) + b"\x01" + bytes(31) + b"\x01"), B(b"\x00\x01"), 2, shift) == 0     # D, -D
    shifted = out(2 * 2 * fp)
    assert lib.bgls_aggregate_sets(cid, 1, B(sigs[0] + bytes(shift)[:2 * fp] + sigs[1] + bytes(shift)[2 * fp:]), offs([2, 2]), 2, shifted) == 0
    bad = [bytes(shifted)[:2 * fp], bytes(shifted)[2 * fp:]]
    mo = offs([len(m) for m in msgs])
    assert lib.bgls_verify_multi_batch(cid, B(b"".join(sigs)), B(keys), offs(sizes), 2, B(b"".join(msgs)), mo, 1) == 1
    assert lib.bgls_verify_multi_batch(cid, B(b"".join(bad)), B(keys), offs(sizes), 2, B(b"".join(msgs)), mo, 1) == 1       # the gap
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None)[:2] == (1, [1])
    for seed in (SEED, bytes(32), b"\xa5" * 32):
        assert run_combined(lib, cid, fp, sizes, keys, msgs, bad, None, seed=seed)[:2] == (0, [0])
        assert run_combined(lib, cid, fp, sizes, keys, msgs, bad, [2], seed=seed)[:2] == (0, [0])
    assert ms.run_sets(lib, cid, fp, sizes, keys, msgs, bad)[:2] == (0, [0, 0])


def test_infinity(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [2, 0, 1, 3, 0, 0, 0]
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 940 + cid)
    inf = bytes(2 * fp)
    sigs = [inf if c == 0 else s for c, s in zip(sizes, sigs)]
    groups = [4, 3]                                          # a valid group with an empty set inside; a group of empty sets only
    rc, v, gts = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups)
    assert (rc, v) == (2, [1, 1]) and gts == identity(fp) * 2
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None)[:2] == (1, [1])
    sigs[1] = sigs[0]                                        # an empty set with a signature that is not infinity
    rc, v, gts = run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups)
    assert (rc, v) == (1, [0, 1])
    assert gts == want_gts(lib, cid, fp, sizes, keys, msgs, sigs, groups, SEED)
    sigs[5] = sigs[0]
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups)[:2] == (0, [0, 0])


def test_whole_call_errors(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [3, 1, 40, 2] + [1] * 66
    groups = [4, 66]
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 950 + cid)
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups)[:2] == (2, [1, 1])
    off_curve = bytearray(sigs[69])
    off_curve[-1] ^= 1
    for g in (groups, None):
        assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs[:69] + [bytes(off_curve)], g)[0] == ERR_ENCODING
        assert run_combined(lib, cid, fp, sizes, keys, msgs, [b"\xff" * (2 * fp)] + sigs[1:], g)[0] == ERR_ENCODING        # non-canonical
        bad = bytearray(keys)
        bad[14 * 4 * fp:15 * 4 * fp] = b"\xff" * (4 * fp)
        assert run_combined(lib, cid, fp, sizes, bytes(bad), msgs, sigs, g)[0] == ERR_ENCODING
        bad = bytearray(keys)
        bad[5 * 4 * fp - 1] ^= 1                              # an off-curve key
        assert run_combined(lib, cid, fp, sizes, bytes(bad), msgs, sigs, g)[0] == ERR_ENCODING
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, [4, 65])[0] == ERR_ARG


def launches(lib, stage):
    t, cnt = ctypes.c_double(), ctypes.c_ulonglong()
    assert lib.bgls_profile_get(stage.encode(), ctypes.byref(t), ctypes.byref(cnt)) == 0
    return cnt.value


def test_device_form_modes_and_profile_scopes(gpu_lib, curve):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [1 + (b % 4) for b in range(150)]
    groups = [64, 0, 61, 25]
    L = 24
    rnd = random.Random(960 + cid)
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 961 + cid, msgs=[rnd.randbytes(L) for _ in sizes])
    sigs[70] = sigs[71]
    dev = torch.device("cuda:0")
    d_sigs = torch.tensor(list(b"".join(sigs)), dtype=torch.uint8, device=dev)
    d_keys = torch.tensor(list(keys), dtype=torch.uint8, device=dev)
    d_msgs = torch.tensor(list(b"".join(msgs)), dtype=torch.uint8, device=dev)
    d_off = torch.tensor(list(offs(sizes)), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def run_dev(g):
        ng = 1 if g is None else len(g)
        v, gt = out(ng), out(ng * 12 * fp)
        rc = lib.bgls_verify_multi_sets_combined_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), len(sizes), max(sizes), d_msgs.data_ptr(), L, L,
                                                     None if g is None else offs(g), ng, B(SEED), v, gt, None)
        return rc, list(v)[:ng], bytes(gt)[:ng * 12 * fp]

    results = []
    try:
        for mode in (0, 1, 2):
            assert lib.bgls_set_throughput_mode(mode) == 0
            results.append((run_combined(lib, cid, fp, sizes, keys, msgs, sigs, groups), run_dev(groups), run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None),
                            run_dev(None)))
    finally:
        lib.bgls_set_throughput_mode(0)
    host, devr, host1, dev1 = results[0]
    assert host[:2] == (3, [1, 1, 0, 1]) and host1[:2] == (0, [0])
    assert devr == host and dev1 == host1
    assert results[1] == results[0] and results[2] == results[0]
    assert lib.bgls_verify_multi_sets_combined_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), len(sizes), 3, d_msgs.data_ptr(), L, L,
                                                   None, 1, B(SEED), out(1), None, None) == ERR_ARG          # a set above max_set
    stages = ("sum_points", "h2c", "rlc", "miller", "final_exp")
    for g, call in ((groups, run_dev), (None, run_dev), (groups, lambda g: run_combined(lib, cid, fp, sizes, keys, msgs, sigs, g, want_gt=False))):
        try:
            assert lib.bgls_profile_enable(1) == 0
            assert call(g)[0] == (3 if g else 0)
            assert {s: launches(lib, s) for s in stages} == {s: 1 for s in stages}, g
            if g:
                assert launches(lib, "epilogue") == 1
        finally:
            lib.bgls_profile_enable(0)


def _points(cv, fp, sizes, keys, sigs):
    from bgls_amd.curves import Point, G1, G2
    at, ks = 0, []
    for c in sizes:
        ks.append([Point(cv, G2, keys[i * 4 * fp:(i + 1) * 4 * fp]) for i in range(at, at + c)])
        at += c
    return [Point(cv, G1, s) for s in sigs], ks


def test_4096_one_key_sets_and_the_located_fallback(gpu_lib, curve, monkeypatch):
    from bgls_amd import Altbn128, Bls12, bgls
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Altbn128 if cid == 0 else Bls12
    n = 1 << 12
    sizes = [1] * n
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 970 + cid)
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None, want_gt=False)[:2] == (1, [1])
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, [64] * 64, want_gt=False)[:2] == (64, [1] * 64)
    sigs[1000] = sigs[1001]
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, None, want_gt=False)[:2] == (0, [0])
    assert run_combined(lib, cid, fp, sizes, keys, msgs, sigs, [64] * 64, want_gt=False)[1] == [int(g != 1000 // 64) for g in range(64)]
    ps, ks = _points(cv, fp, sizes, keys, sigs)
    want = bgls.VerifyMultiSignatures(cv, ps, ks, msgs)
    assert want == [b != 1000 for b in range(n)]
    per_set, plain = [], bgls.VerifyMultiSignatures
    monkeypatch.setattr(bgls, "VerifyMultiSignatures", lambda c, a, k, m: per_set.append(len(a)) or plain(c, a, k, m))
    try:
        assert lib.bgls_profile_enable(1) == 0
        got = bgls.VerifyMultiSignaturesLocated(cv, ps, ks, msgs)
        # one combined call, then ONE per-set call over the 64 sets of the rejected group, not over 4096
        assert launches(lib, "final_exp") == 2 and launches(lib, "rlc") == 1 and launches(lib, "h2c") == 2
    finally:
        lib.bgls_profile_enable(0)
    assert got == want and per_set == [64]


def test_python_mirrors(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Altbn128 if cid == 0 else Bls12
    sizes = [2, 0, 1, 5, 1, 3, 2]
    keys, msgs, sigs, _ = ms.make_sets(lib, cid, fp, sizes, 980 + cid)
    sigs[1] = bytes(2 * fp)
    ps, ks = _points(cv, fp, sizes, keys, sigs)
    assert bgls.VerifyMultiSignaturesCombined(cv, ps, ks, msgs) == [True]
    assert bgls.VerifyMultiSignaturesCombined(cv, ps, ks, msgs, group=3, seed=SEED) == [True, True, True]
    assert bgls.VerifyMultiSignaturesLocated(cv, ps, ks, msgs, group=2) == [True] * 7
    assert bgls.VerifyMultiSignaturesCombined(cv, [], [], []) == []
    ps[4] = ps[0]
    assert bgls.VerifyMultiSignaturesCombined(cv, ps, ks, msgs) == [False]
    assert bgls.VerifyMultiSignaturesCombined(cv, ps, ks, msgs, group=3) == [True, False, True]
    assert bgls.VerifyMultiSignaturesLocated(cv, ps, ks, msgs, group=3) == bgls.VerifyMultiSignatures(cv, ps, ks, msgs) == [b != 4 for b in range(7)]
    # the 0x01 prefix: signatures made over the prefixed messages
    keys2, pm, sigs2, _ = ms.make_sets(lib, cid, fp, sizes, 981 + cid, msgs=[b"\x01" + m for m in msgs])
    sigs2[1] = bytes(2 * fp)
    ps2, ks2 = _points(cv, fp, sizes, keys2, sigs2)
    assert bgls.KoskVerifyMultiSignaturesCombined(cv, ps2, ks2, msgs, group=4) == [True, True]
    assert bgls.VerifyMultiSignaturesCombined(cv, ps2, ks2, msgs, group=4) == [False, False]
    with pytest.raises(ValueError):
        bgls.VerifyMultiSignaturesCombined(cv, ps, ks, msgs, seed=b"short")
    with pytest.raises(ValueError):
        bgls.VerifyMultiSignaturesCombined(cv, [None] + ps[1:], ks, msgs)
