"""GPU tier: n_sets VerifyMultiSignatureWithHAE calls (bgls/blsHAE.go:56-58) in one set of launches (bgls_verify_multi_hae_sets / _dev) and
the per-set exponents (bgls_hae_exponents_sets): exponents against the single call and the C oracle over ragged sizes with the roots on
the host and on the device, verdicts against bgls_verify_multi_hae and the oracle on a mixed batch, the key sums against
bgls_weighted_sum_dev, the GT elements against bgls_verify_multi_sets, 2^13 sets of 128 keys, whole-call errors, the device form, the
profile scopes and the Python mirror."""
import ctypes
import json
import os
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE_MAX = (1 << 64) - 1
HOST_MIN_DEFAULT = 2048


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offs(counts, base=0):
    o = (ctypes.c_uint64 * (len(counts) + 1))(base)
    for i, c in enumerate(counts):
        o[i + 1] = o[i] + c
    return o


@pytest.fixture
def host_min(gpu_lib, request):
    assert gpu_lib.bgls_set_hae_root_host_min(request.param) == 0
    yield request.param
    gpu_lib.bgls_set_hae_root_host_min(HOST_MIN_DEFAULT)


def gen_keys(lib, cid, fp, n, seed):
    rnd = random.Random(seed)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n)]
    keys = out(n * 4 * fp)
    if n:
        assert lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), n, keys) == 0
    return sks, bytes(keys)[:n * 4 * fp]


def split(keys, sizes, fp):
    res, at = [], 0
    for c in sizes:
        res.append(keys[at * 4 * fp:(at + c) * 4 * fp])
        at += c
    return res


def hae_sign(lib, cid, fp, sks, kb, msg):
    """AggregateSignaturesWithHAE over Sign(sk_i, msg) (bgls/blsHAE.go:39-46)"""
    n = len(sks)
    if n == 0:
        return bytes(2 * fp)
    sigs = out(n * 2 * fp)
    assert lib.bgls_sign_batch(cid, B(b"".join(s.to_bytes(32, "big") for s in sks)), B(msg * n), offs([len(msg)] * n), n, sigs) == 0
    agg = out(2 * fp)
    assert lib.bgls_aggregate_signatures_hae(cid, sigs, B(kb), n, agg) == 0
    return bytes(agg)


def run_hae(lib, cid, fp, key_sets, msgs, sigs):
    nb = len(key_sets)
    v, apk, gt = out(nb), out(nb * 4 * fp), out(nb * 12 * fp)
    rc = lib.bgls_verify_multi_hae_sets(cid, B(b"".join(sigs)), B(b"".join(key_sets)), offs([len(k) // (4 * fp) for k in key_sets]), nb,
                                        B(b"".join(msgs)), offs([len(m) for m in msgs]), v, apk, gt)
    return rc, list(v)[:nb], bytes(apk), bytes(gt)


def single_exponents(lib, cid, kb, n):
    t = out(16 * n)
    assert lib.bgls_hae_exponents(cid, B(kb), n, t) == 0
    return bytes(t)[:16 * n]


@pytest.mark.parametrize("host_min", [0, SIZE_MAX], indirect=True)
def test_exponents_match_single_call_and_oracle(gpu_lib, curve, host_min):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 4100, 7]
    _, keys = gen_keys(lib, cid, fp, sum(sizes), 5 + cid)
    t = out(16 * sum(sizes))
    assert lib.bgls_hae_exponents_sets(cid, B(keys), offs(sizes), len(sizes), t) == 0
    t = bytes(t)
    at = 0
    for c, kb in zip(sizes, split(keys, sizes, fp)):
        got = t[16 * at:16 * (at + c)]
        assert got == single_exponents(lib, cid, kb, c), c
        assert [int.from_bytes(got[16 * i:16 * i + 16], "big") for i in range(c)] == coracle.hae_exponents(cid, kb, c), c
        at += c
    # offsets that do not start at 0: set b's exponents at 16 key_off[b] of t_out
    t2 = out(16 * (3 + 9))
    assert lib.bgls_hae_exponents_sets(cid, B(bytes(3 * 4 * fp) + keys[:9 * 4 * fp]), offs([4, 5], base=3), 2, t2) == 0
    assert bytes(t2)[48:48 + 64] == single_exponents(lib, cid, keys[:4 * 4 * fp], 4)
    assert bytes(t2)[112:] == single_exponents(lib, cid, keys[4 * 4 * fp:9 * 4 * fp], 5)


def mixed_batch(lib, cid, fp, seed):
    """valid HAE multi-signatures of ragged sizes and the tampered forms: (key sets, messages, signatures, what each set is)"""
    rnd = random.Random(seed)
    sizes = [3, 1, 5, 64, 2, 33, 4, 6, 3, 2, 0]
    sks, keys = gen_keys(lib, cid, fp, sum(sizes), seed)
    ksets = split(keys, sizes, fp)
    sk_sets, at = [], 0
    for c in sizes:
        sk_sets.append(sks[at:at + c])
        at += c
    msgs = [rnd.randbytes(1 + rnd.randrange(40)) for _ in sizes]
    sigs = [hae_sign(lib, cid, fp, s, k, m) for s, k, m in zip(sk_sets, ksets, msgs)]
    K = 4 * fp
    names = ["valid"] * 6 + ["flipped bit", "swapped keys", "dropped key", "other signature", "empty"]
    msgs[6] = bytes([msgs[6][0] ^ 1]) + msgs[6][1:]
    ksets[7] = ksets[7][K:2 * K] + ksets[7][:K] + ksets[7][2 * K:]           # the same keys in another order: other weights
    ksets[8] = ksets[8][:2 * K]                                              # a signer dropped
    sigs[9] = sigs[0]
    sigs[10] = bytes(2 * fp)
    # a repeated key, signed with it twice: accepted as by the single call
    rep_k = ksets[0][:K] + ksets[0][K:2 * K] + ksets[0][:K]
    ksets.append(rep_k)
    msgs.append(b"repeated")
    sigs.append(hae_sign(lib, cid, fp, [sk_sets[0][0], sk_sets[0][1], sk_sets[0][0]], rep_k, b"repeated"))
    names.append("repeated key")
    return ksets, msgs, sigs, names


def subgroup_sets(curve, ksets, msgs, sigs):
    """keys and signatures on the curve outside the order-r subgroup (tests/golden), which the Verify* calls do not reject"""
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "subgroup_%s.json" % curve["name"])))
    g2_off = [bytes.fromhex(p["pt"]) for p in fix["points"] if p.get("on_twist") and not p.get("in_subgroup") and not p.get("miller_degenerates")]
    g1_off = [bytes.fromhex(p["pt"]) for p in fix.get("g1_points", []) if p.get("on_curve") and not p.get("in_subgroup")]
    assert g2_off
    ks, ms, ss = [], [], []
    for k in g2_off:
        ks += [k, ksets[1] + k]
        ms += [msgs[1], msgs[1]]
        ss += [sigs[1], sigs[1]]
    for s in g1_off:
        ks.append(ksets[1])
        ms.append(msgs[1])
        ss.append(s)
    return ks, ms, ss


@pytest.mark.parametrize("host_min", [0, SIZE_MAX], indirect=True)
def test_mixed_batch_matches_single_calls(gpu_lib, curve, host_min):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    ksets, msgs, sigs, names = mixed_batch(lib, cid, fp, 31 + cid)
    ks, ms, ss = subgroup_sets(curve, ksets, msgs, sigs)
    ksets, msgs, sigs = ksets + ks, msgs + ms, sigs + ss
    nb = len(ksets)
    rc, verdicts, apks, gts = run_hae(lib, cid, fp, ksets, msgs, sigs)
    assert rc == sum(verdicts) and rc >= 0
    for b in range(nb):
        n = len(ksets[b]) // (4 * fp)
        want = lib.bgls_verify_multi_hae(cid, B(sigs[b]), B(ksets[b]), n, B(msgs[b]), len(msgs[b]))
        assert want in (0, 1)
        assert verdicts[b] == want, b
        assert coracle.verify_multi_hae(cid, sigs[b], ksets[b], n, msgs[b]) == want, b
    expect = {"valid": 1, "flipped bit": 0, "swapped keys": 0, "dropped key": 0, "other signature": 0, "repeated key": 1}
    for b, name in enumerate(names):
        if name in expect:
            assert verdicts[b] == expect[name], name
    # apk_out: byte-equal to getAggregatePubKey over the single path's exponents (bgls_weighted_sum_dev)
    dev = torch.device("cuda:0")
    for b in range(nb):
        n = len(ksets[b]) // (4 * fp)
        d_pts = torch.tensor(list(ksets[b] or b"\0"), dtype=torch.uint8, device=dev)
        d_w = torch.tensor(list(single_exponents(lib, cid, ksets[b], n) or b"\0"), dtype=torch.uint8, device=dev)
        d_out = torch.zeros(4 * fp, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert lib.bgls_weighted_sum_dev(cid, 2, d_pts.data_ptr(), d_w.data_ptr(), n, d_out.data_ptr(), None) == 0
        assert bytes(d_out.cpu().tolist()) == apks[b * 4 * fp:(b + 1) * 4 * fp], b
    # gt_out: byte-equal to bgls_verify_multi_sets' GT element of the one-key sets {apk_b}
    v1, gt1 = out(nb), out(nb * 12 * fp)
    rc1 = lib.bgls_verify_multi_sets(cid, B(b"".join(sigs)), B(apks), offs([1] * nb), nb, B(b"".join(msgs)), offs([len(m) for m in msgs]), v1, gt1)
    assert rc1 == rc and list(v1)[:nb] == verdicts and bytes(gt1) == gts


def test_2_13_sets_of_128_keys(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    r = (Altbn128 if cid == 0 else Bls12).GetG1Order()
    n_sets, k = 1 << 13, 128
    sks, keys = gen_keys(lib, cid, fp, n_sets * k, 11 + cid)
    t = out(16 * n_sets * k)
    assert lib.bgls_hae_exponents_sets(cid, B(keys), offs([k] * n_sets), n_sets, t) == 0
    t = bytes(t)
    # the HAE aggregate of set b is (sum_i t_i sk_i) H(m_b): one signing call for all sets
    agg_sk = []
    for b in range(n_sets):
        acc = 0
        for i in range(b * k, (b + 1) * k):
            acc += int.from_bytes(t[16 * i:16 * i + 16], "big") * sks[i]
        agg_sk.append(acc % r)
    msgs = [b"committee %d" % b for b in range(n_sets)]
    sg = out(n_sets * 2 * fp)
    assert lib.bgls_sign_batch(cid, B(b"".join(s.to_bytes(32, "big") for s in agg_sk)), B(b"".join(msgs)), offs([len(m) for m in msgs]), n_sets, sg) == 0
    sigs = [bytes(sg)[b * 2 * fp:(b + 1) * 2 * fp] for b in range(n_sets)]
    ksets = split(keys, [k] * n_sets, fp)
    rc, verdicts, _, _ = run_hae(lib, cid, fp, ksets, msgs, sigs)
    assert rc == n_sets and all(v == 1 for v in verdicts)
    bad = [5, 4000, n_sets - 1]
    msgs[5] = b"tampered"
    ksets[4000] = ksets[4000][4 * fp:8 * fp] + ksets[4000][:4 * fp] + ksets[4000][8 * fp:]
    sigs[n_sets - 1] = sigs[0]
    rc, verdicts, _, _ = run_hae(lib, cid, fp, ksets, msgs, sigs)
    assert rc == n_sets - len(bad)
    assert [b for b in range(n_sets) if verdicts[b] != 1] == bad
    for b in (0, 5, 4000, n_sets - 1):
        assert lib.bgls_verify_multi_hae(cid, B(sigs[b]), B(ksets[b]), k, B(msgs[b]), len(msgs[b])) == verdicts[b], b


def test_errors_device_form_and_profile_scopes(gpu_lib, curve):
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [3, 0, 1, 40, 2, 5]
    sks, keys = gen_keys(lib, cid, fp, sum(sizes), 23 + cid)
    L = 24
    rnd = random.Random(cid)
    msgs = [rnd.randbytes(L) for _ in sizes]
    ksets = split(keys, sizes, fp)
    sk_sets, at = [], 0
    for c in sizes:
        sk_sets.append(sks[at:at + c])
        at += c
    sigs = [hae_sign(lib, cid, fp, s, kb, m) for s, kb, m in zip(sk_sets, ksets, msgs)]
    sigs[4] = sigs[3]
    nb = len(sizes)
    rc, verdicts, apks, gts = run_hae(lib, cid, fp, ksets, msgs, sigs)
    assert rc == 5 and verdicts == [1, 1, 1, 1, 0, 1]
    # an off-curve key in one set fails the whole call with the single call's code
    badk = bytearray(ksets[3])
    badk[10 * 4 * fp + 5] ^= 1
    single_rc = lib.bgls_verify_multi_hae(cid, B(sigs[3]), B(bytes(badk)), 40, B(msgs[3]), L)
    assert single_rc == ERR_ENCODING
    assert run_hae(lib, cid, fp, ksets[:3] + [bytes(badk)] + ksets[4:], msgs, sigs)[0] == single_rc
    # the device form (fixed-stride messages) agrees with the host form
    dev = torch.device("cuda:0")
    d_sigs = torch.tensor(list(b"".join(sigs)), dtype=torch.uint8, device=dev)
    d_keys = torch.tensor(list(keys), dtype=torch.uint8, device=dev)
    d_msgs = torch.tensor(list(b"".join(msgs)), dtype=torch.uint8, device=dev)
    d_off = torch.tensor(list(offs(sizes)), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    v2, apk2, gt2 = out(nb), out(nb * 4 * fp), out(nb * 12 * fp)
    rc2 = lib.bgls_verify_multi_hae_sets_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), nb, max(sizes), d_msgs.data_ptr(), L, L,
                                             v2, apk2, gt2, None)
    assert rc2 == rc and list(v2)[:nb] == verdicts and bytes(apk2) == apks and bytes(gt2) == gts
    assert lib.bgls_verify_multi_hae_sets_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), nb, 39, d_msgs.data_ptr(), L, L,
                                              v2, None, None, None) == ERR_ARG

    def launches(stage):
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        assert lib.bgls_profile_get(stage.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0
        return cnt.value

    try:
        assert lib.bgls_profile_enable(1) == 0
        assert run_hae(lib, cid, fp, ksets, msgs, sigs)[0] == 5
        assert {s: launches(s) for s in ("hae_keys", "final_exp", "sum_points")} == {"hae_keys": 1, "final_exp": 1, "sum_points": 1}
        assert lib.bgls_profile_enable(1) == 0
        assert lib.bgls_verify_multi_hae_sets_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), d_off.data_ptr(), nb, max(sizes), d_msgs.data_ptr(), L, L,
                                                  v2, None, None, None) == 5
        assert (launches("hae_keys"), launches("final_exp")) == (1, 1)
    finally:
        lib.bgls_profile_enable(0)


def test_python_mirror(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    from bgls_amd.curves import Point, G1, G2
    cv = Altbn128 if curve["id"] == 0 else Bls12
    other = Bls12 if curve["id"] == 0 else Altbn128
    rnd = random.Random(97 + curve["id"])
    # the reference's TestMultiSigWithHAE (bgls/blsHAE_test.go:56-82) as one batch: 5 tests of 8 signers -- valid, on another message, and
    # with a foreign signer in place of the first
    aggs, signers, msgs = [], [], []
    for _ in range(5):
        msg = rnd.randbytes(32)
        keys = [bgls.KeyGen(cv) for _ in range(8)]
        s = [k[1] for k in keys]
        agg = bgls.AggregateSignaturesWithHAE([bgls.Sign(cv, k[0], msg) for k in keys], s)
        aggs += [agg, agg, agg]
        signers += [s, s, [bgls.KeyGen(cv)[1]] + s[1:]]
        msgs += [msg, rnd.randbytes(32), msg]
    got = bgls.VerifyMultiSignaturesWithHAE(cv, aggs, signers, msgs)
    assert got == [True, False, False] * 5
    assert got == [bgls.VerifyMultiSignatureWithHAE(cv, a, s, m) for a, s, m in zip(aggs, signers, msgs)]
    # a nil signature and another curve's key are settled alone
    aggs2, signers2 = list(aggs[:3]), list(signers[:3])
    aggs2[1] = None
    signers2[2] = [Point(other, G2, other.GetG2().raw)]
    assert bgls.VerifyMultiSignaturesWithHAE(cv, aggs2, signers2, msgs[:3]) == [True, False, False]
    # a whole-call error (a non-canonical key in set 1) is settled set by set
    bad = [signers[0], signers[0][:7] + [Point(cv, G2, b"\xff" * len(signers[0][0].raw))], signers[0]]
    assert bgls.VerifyMultiSignaturesWithHAE(cv, [aggs[0]] * 3, bad, [msgs[0], msgs[0], msgs[1]]) == [True, False, False]
    assert bgls.VerifyMultiSignaturesWithHAE(cv, [Point(cv, G1, aggs[0].raw)], [signers[0]], [msgs[0]]) == [True]
