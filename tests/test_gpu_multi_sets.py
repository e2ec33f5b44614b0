"""GPU tier: n_sets independent verifyMultiSignature calls (bgls/bgls.go:89-92) in one set of launches (bgls_verify_multi_sets / _dev):
every verdict and GT element against bgls_verify_multi on that set alone, ragged set sizes, set counts around k_miller_sets' 30 sets
per block, 2^16 one-key sets (batched VerifySingleSignature), the subgroup fixtures as keys and signatures, whole-call errors, the
device form, the throughput modes, one profile scope per stage and the Python mirrors."""
import ctypes
import json
import os
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPB = 30                                                  # k_miller_sets: sets per block
ROUND = 768 * SPB                                         # one round of resident blocks: three blocks per CU on 256 CUs


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offs(counts):
    o = (ctypes.c_uint64 * (len(counts) + 1))()
    for i, c in enumerate(counts):
        o[i + 1] = o[i] + c
    return o


def make_sets(lib, cid, fp, sizes, seed, msgs=None):
    """len(sizes) valid multi-signatures: set b has sizes[b] signers of one message.  Returns (flat keys, messages, signatures,
    one spare key of a signer outside every set)."""
    rnd = random.Random(seed)
    n = sum(sizes)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n + 1)]
    kb = b"".join(s.to_bytes(32, "big") for s in sks)
    keys = out((n + 1) * 4 * fp)
    assert lib.bgls_scale_generator(cid, 2, B(kb), n + 1, keys) == 0
    if msgs is None:
        msgs = [rnd.randbytes(1 + rnd.randrange(40)) for _ in sizes]
    per_key = [msgs[b] for b, c in enumerate(sizes) for _ in range(c)]
    sigs = out(max(n, 1) * 2 * fp)
    if n:
        assert lib.bgls_sign_batch(cid, B(kb[:32 * n]), B(b"".join(per_key)), offs([len(m) for m in per_key]), n, sigs) == 0
    aggs = out(len(sizes) * 2 * fp)
    assert lib.bgls_aggregate_sets(cid, 1, sigs, offs(sizes), len(sizes), aggs) == 0
    keys = bytes(keys)
    return keys[:n * 4 * fp], list(msgs), [bytes(aggs)[b * 2 * fp:(b + 1) * 2 * fp] for b in range(len(sizes))], keys[n * 4 * fp:]


def run_sets(lib, cid, fp, sizes, keys, msgs, sigs, want_gt=True):
    nb = len(sizes)
    verdicts = out(nb)
    gt = out(nb * 12 * fp) if want_gt else None
    rc = lib.bgls_verify_multi_sets(cid, B(b"".join(sigs)), B(keys), offs(sizes), nb, B(b"".join(msgs)), offs([len(m) for m in msgs]), verdicts, gt)
    return rc, list(verdicts)[:nb], (bytes(gt) if want_gt else None)


def single(lib, cid, sig, keys, n, msg):
    return lib.bgls_verify_multi(cid, B(sig), B(keys), n, B(msg), len(msg))


def single_gt(lib, cid, fp, sig, keys, n, msg):
    """the single path's GT element e(-sig, g2) e(H(m), apk): the key sum, then a one-key set through bgls_verify_aggregate_h_gt"""
    apk = out(4 * fp)
    assert lib.bgls_aggregate_sets(cid, 2, B(keys), offs([n]), 1, apk) == 0
    h = ctypes.c_uint64()
    devs = (ctypes.c_int * 1)(0)
    assert lib.bgls_keys_upload(cid, apk, 1, devs, 1, 0, ctypes.byref(h)) == 0
    gt = out(12 * fp)
    rc = lib.bgls_verify_aggregate_h_gt(h, B(sig), B(msg), offs([len(msg)]), 1, 1, gt)
    assert lib.bgls_keys_free(h) == 0
    assert rc in (0, 1)
    return bytes(gt)


def check_against_single(lib, cid, fp, sizes, keys, msgs, sigs, verdicts, gts, gt_every=1):
    at = 0
    for b, c in enumerate(sizes):
        kb = keys[at * 4 * fp:(at + c) * 4 * fp]
        want = single(lib, cid, sigs[b], kb, c, msgs[b])
        assert want in (0, 1)
        assert verdicts[b] == want, (b, c)
        if gts is not None and b % gt_every == 0:
            assert gts[b * 12 * fp:(b + 1) * 12 * fp] == single_gt(lib, cid, fp, sigs[b], kb, c, msgs[b]), (b, c)
        at += c


SIZES = [0, 1, 2, 127, 128, 129, 1000]


def test_ragged_sets_match_single_calls(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = SIZES + [1, 5, 3, 0, 2]
    keys, msgs, sigs, spare = make_sets(lib, cid, fp, sizes, 41 + cid)
    keys, sigs, msgs = bytearray(keys), list(sigs), list(msgs)
    starts = [sum(sizes[:b]) for b in range(len(sizes))]
    msgs[8] = msgs[8] + b"x"                              # wrong message
    sigs[9] = sigs[7]                                     # wrong signature
    keys[(starts[2] + 1) * 4 * fp:(starts[2] + 2) * 4 * fp] = spare      # a key swapped for one outside the set
    sigs[10] = bytes(2 * fp)                              # an empty set with the infinity signature: accepted
    sigs[0] = sigs[1]                                     # an empty set with a signature that is not infinity: refused
    keys = bytes(keys)
    rc, verdicts, gts = run_sets(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == sum(verdicts) and rc >= 0
    assert verdicts == [0, 1, 0, 1, 1, 1, 1, 1, 0, 0, 1, 1]
    check_against_single(lib, cid, fp, sizes, keys, msgs, sigs, verdicts, gts)
    # spot checks against the C oracle
    for b in (1, 3, 8, 9):
        kb = keys[starts[b] * 4 * fp:(starts[b] + sizes[b]) * 4 * fp]
        assert coracle.verify_multi(cid, sigs[b], kb, sizes[b], msgs[b]) == verdicts[b], b


@pytest.mark.parametrize("n_sets", [1, SPB - 1, SPB, SPB + 1, ROUND - 1, ROUND, ROUND + 1])
def test_set_counts_around_blocks_and_rounds(gpu_lib, curve, n_sets):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(n_sets)
    sizes = [1 + rnd.randrange(3) for _ in range(n_sets)]
    shared = [b"same message"] * n_sets                   # the same message in every set: no duplicate rule
    msgs = shared if n_sets % 2 else None
    keys, msgs, sigs, _ = make_sets(lib, cid, fp, sizes, 7 * n_sets + cid, msgs=msgs)
    bad = sorted({0, n_sets // 2, n_sets - 1})
    for b in bad:
        msgs[b] = msgs[b] + b"!"
    rc, verdicts, gts = run_sets(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == n_sets - len(bad)
    assert [b for b in range(n_sets) if verdicts[b] != 1] == bad
    if n_sets <= 64:
        check_against_single(lib, cid, fp, sizes, keys, msgs, sigs, verdicts, gts)
    else:
        at = 0
        for b in range(n_sets):
            if b in bad or b in (1, SPB, ROUND - 2, n_sets - 2):
                kb = keys[at * 4 * fp:(at + sizes[b]) * 4 * fp]
                assert verdicts[b] == single(lib, cid, sigs[b], kb, sizes[b], msgs[b]), b
                assert gts[b * 12 * fp:(b + 1) * 12 * fp] == single_gt(lib, cid, fp, sigs[b], kb, sizes[b], msgs[b]), b
            at += sizes[b]


def test_2_16_single_signatures(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 1 << 16
    sizes = [1] * n
    keys, msgs, sigs, _ = make_sets(lib, cid, fp, sizes, 3 + cid)
    sigs[777] = sigs[778]
    rc, verdicts, gts = run_sets(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == n - 1 and verdicts[777] == 0 and sum(verdicts) == n - 1
    for b in (0, 777, 40000, n - 1):
        kb = keys[b * 4 * fp:(b + 1) * 4 * fp]
        assert verdicts[b] == single(lib, cid, sigs[b], kb, 1, msgs[b]), b
        assert gts[b * 12 * fp:(b + 1) * 12 * fp] == single_gt(lib, cid, fp, sigs[b], kb, 1, msgs[b]), b


def test_subgroup_fixtures_as_keys_and_signatures(gpu_lib, curve):
    """points on the curve but outside the order-r subgroup, which the Verify* calls do not reject: verdicts and GT bytes still equal
    the single path's (on BLS12-381 that needs its order: the hash pair's Miller value raised to h before the signature pair)"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "subgroup_%s.json" % curve["name"])))
    g2_off = [bytes.fromhex(p["pt"]) for p in fix["points"] if p.get("on_twist") and not p.get("in_subgroup") and not p.get("miller_degenerates")]
    g1_off = [bytes.fromhex(p["pt"]) for p in fix.get("g1_points", []) if p.get("on_curve") and not p.get("in_subgroup")]
    assert g2_off
    base_sizes = [2, 1, 3, 1]
    keys, msgs, sigs, _ = make_sets(lib, cid, fp, base_sizes, 19 + cid)
    sizes, kl, sl, ml = [], [], [], []
    at = 0
    for b, c in enumerate(base_sizes):                    # the valid sets, as made
        sizes.append(c)
        kl.append(keys[at * 4 * fp:(at + c) * 4 * fp])
        sl.append(sigs[b])
        ml.append(msgs[b])
        at += c
    for i, k in enumerate(g2_off):                        # an off-subgroup key alone and beside a real key
        sizes += [1, 2]
        kl += [k, kl[1] + k]
        sl += [sigs[1], sigs[1]]
        ml += [msgs[1], msgs[1]]
    for s in g1_off:                                      # an off-subgroup signature
        sizes.append(1)
        kl.append(kl[1])
        sl.append(s)
        ml.append(msgs[1])
    flat = b"".join(kl)
    rc, verdicts, gts = run_sets(lib, cid, fp, sizes, flat, ml, sl)
    assert rc >= 0
    check_against_single(lib, cid, fp, sizes, flat, ml, sl, verdicts, gts)


def test_whole_call_errors_and_device_form(gpu_lib, curve):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [3, 0, 1, 40, 2]
    keys, msgs, sigs, _ = make_sets(lib, cid, fp, sizes, 23 + cid)
    sigs[1] = bytes(2 * fp)
    sigs[4] = sigs[3]
    nb = len(sizes)
    rc, verdicts, gts = run_sets(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == 4 and verdicts == [1, 1, 1, 1, 0]
    # a non-canonical key in one set fails the whole call
    bad = bytearray(keys)
    bad[(4 + 10) * 4 * fp:(4 + 11) * 4 * fp] = b"\xff" * (4 * fp)
    assert run_sets(lib, cid, fp, sizes, bytes(bad), msgs, sigs)[0] == ERR_ENCODING
    # offsets not monotone; an empty batch
    v = out(nb)
    arr = (ctypes.c_uint64 * 6)(0, 3, 2, 4, 44, 46)
    assert lib.bgls_verify_multi_sets(cid, B(b"".join(sigs)), B(keys), arr, nb, B(b"".join(msgs)), offs([len(m) for m in msgs]), v, None) == ERR_ARG
    assert lib.bgls_verify_multi_sets(cid, None, None, offs([]), 0, None, offs([]), None, None) == 0
    # the device form (fixed-stride messages): same verdicts and GT bytes as the host form on the same sets
    L = 24
    fmsgs = [(m * L)[:L] if m else bytes(L) for m in msgs]
    keys2, fmsgs, sigs2, _ = make_sets(lib, cid, fp, sizes, 29 + cid, msgs=fmsgs)
    sigs2[1] = bytes(2 * fp)
    sigs2[4] = sigs2[3]
    rc1, v1, gt1 = run_sets(lib, cid, fp, sizes, keys2, fmsgs, sigs2)
    dev = torch.device("cuda:0")
    d_sigs = torch.tensor(list(b"".join(sigs2)), dtype=torch.uint8, device=dev)
    d_keys = torch.tensor(list(keys2), dtype=torch.uint8, device=dev)
    d_msgs = torch.tensor(list(b"".join(fmsgs)), dtype=torch.uint8, device=dev)
    d_off = torch.tensor(list(offs(sizes)), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    v2, gt2 = out(nb), out(nb * 12 * fp)
    rc2 = lib.bgls_verify_multi_sets_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), nb, max(sizes), d_msgs.data_ptr(), L, L, v2, gt2, None)
    assert rc2 == rc1 == 4 and list(v2)[:nb] == v1 and bytes(gt2) == gt1
    # device offsets above max_set or not monotone are refused
    assert lib.bgls_verify_multi_sets_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), nb, 39, d_msgs.data_ptr(), L, L, v2, None, None) == ERR_ARG
    d_bad = torch.tensor([0, 3, 2, 4, 44, 46], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert lib.bgls_verify_multi_sets_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_bad.data_ptr(), nb, 64, d_msgs.data_ptr(), L, L, v2, None, None) == ERR_ARG


def test_throughput_modes_and_profile_scopes(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [1 + (b % 7) for b in range(100)]
    keys, msgs, sigs, _ = make_sets(lib, cid, fp, sizes, 61 + cid)
    sigs[5] = sigs[6]
    results = []
    try:
        for mode in (0, 1, 2):
            assert lib.bgls_set_throughput_mode(mode) == 0
            results.append(run_sets(lib, cid, fp, sizes, keys, msgs, sigs))
    finally:
        lib.bgls_set_throughput_mode(0)
    assert results[0][0] == 99 and results[1] == results[0] and results[2] == results[0]

    def launches(stage):
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        assert lib.bgls_profile_get(stage.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0
        return cnt.value

    try:
        assert lib.bgls_profile_enable(1) == 0
        assert run_sets(lib, cid, fp, sizes, keys, msgs, sigs, want_gt=False)[0] == 99
        want = {"sum_points": 1, "h2c": 1, "miller": 1, "final_exp": 1, "epilogue": 1 if cid == 1 else 0, "scatter": 0, "reduce": 0, "dup_check": 0}
        assert {s: launches(s) for s in want} == want
    finally:
        lib.bgls_profile_enable(0)


def test_python_mirrors(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    from bgls_amd.curves import Point, G1, G2
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Altbn128 if cid == 0 else Bls12
    sizes = [2, 0, 1, 5]
    keys, msgs, sigs, _ = make_sets(lib, cid, fp, sizes, 83 + cid)
    at, ks = 0, []
    for c in sizes:
        ks.append([Point(cv, G2, keys[i * 4 * fp:(i + 1) * 4 * fp]) for i in range(at, at + c)])
        at += c
    ps = [Point(cv, G1, s) for s in sigs]
    ps[1] = Point(cv, G1, bytes(2 * fp))
    ps[3] = ps[0]
    want = [bgls._verify_multi(cv, s, k, bytes(m)) for s, k, m in zip(ps, ks, msgs)]
    assert want == [True, True, True, False]
    assert bgls.VerifyMultiSignatures(cv, ps, ks, msgs) == want
    assert bgls.KoskVerifyMultiSignatures(cv, ps, ks, msgs) == [bgls.KoskVerifyMultiSignature(cv, s, k, m) for s, k, m in zip(ps, ks, msgs)]
    # a nil signature and a foreign point are settled alone
    other = Bls12 if cid == 0 else Altbn128
    ps2 = [ps[0], None, ps[2], ps[3]]
    ks2 = [ks[0], ks[1], [Point(other, G2, other.GetG2().raw)], ks[3]]
    assert bgls.VerifyMultiSignatures(cv, ps2, ks2, msgs) == [True, False, False, False]
    # a whole-call error (a non-canonical key in set 3) is settled set by set: the other sets keep their single-call answers
    bad = list(ks)
    bad[3] = ks[3][:4] + [Point(cv, G2, b"\xff" * (4 * fp))]
    got = bgls.VerifyMultiSignatures(cv, ps, bad, msgs)
    assert got == [True, True, True, False]
    # single signatures: one key per set
    keys1, msgs1, sigs1, _ = make_sets(lib, cid, fp, [1] * 5, 87 + cid)
    pk = [Point(cv, G2, keys1[i * 4 * fp:(i + 1) * 4 * fp]) for i in range(5)]
    ss = [Point(cv, G1, s) for s in sigs1]
    ss[2] = ss[3]
    want1 = [bgls.VerifySingleSignature(cv, s, k, m) for s, k, m in zip(ss, pk, msgs1)]
    assert want1 == [True, True, False, True, True]
    assert bgls.VerifySingleSignatures(cv, ss, pk, msgs1) == want1
    assert bgls.KoskVerifySingleSignatures(cv, ss, pk, msgs1) == [bgls.KoskVerifySingleSignature(cv, s, k, m) for s, k, m in zip(ss, pk, msgs1)]
