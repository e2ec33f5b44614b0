"""GPU tier: B independent VerifyAggregateSignature calls (bgls/bgls.go:82-84,94-119) in one set of launches
(bgls_verify_aggregate_batch / _dev): every verdict and GT element against the single call on that instance alone, ragged instance
sizes around the Miller kernel's six-pairing groups and 60-pairing blocks, the 16 x 2^16 headline shape, one profile scope per
stage for the whole batch, the per-instance scope of the duplicate rule, whole-call errors and the Python mirror."""
import ctypes
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offs(counts):
    o = (ctypes.c_uint64 * (len(counts) + 1))()
    for i, c in enumerate(counts):
        o[i + 1] = o[i] + c
    return o


def make_batch(lib, cid, fp, sizes, seed, dup_in=(), msg_len=32):
    """len(sizes) valid aggregate instances made by the engine: instance b has sizes[b] signers, one message each; in the instances of
    `dup_in` the second message repeats the first BEFORE signing (a valid aggregate that only the duplicate rule refuses).
    Returns (keys, per-key messages, aggregate signatures, one spare key of a signer outside every instance)."""
    rnd = random.Random(seed)
    n = sum(sizes)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n + 1)]
    kb = b"".join(s.to_bytes(32, "big") for s in sks)
    keys = out((n + 1) * 4 * fp)
    assert lib.bgls_scale_generator(cid, 2, B(kb), n + 1, keys) == 0
    msgs = [rnd.randbytes(msg_len) for _ in range(n)]
    at = 0
    for b, c in enumerate(sizes):
        if b in dup_in:
            assert c >= 2
            msgs[at + 1] = msgs[at]
        at += c
    sigs = out(max(n, 1) * 2 * fp)
    if n:
        assert lib.bgls_sign_batch(cid, B(kb[:32 * n]), B(b"".join(msgs)), offs([len(m) for m in msgs]), n, sigs) == 0
    aggs = out(len(sizes) * 2 * fp)
    assert lib.bgls_aggregate_sets(cid, 1, sigs, offs(sizes), len(sizes), aggs) == 0
    keys = bytes(keys)
    return keys[:n * 4 * fp], msgs, [bytes(aggs)[b * 2 * fp:(b + 1) * 2 * fp] for b in range(len(sizes))], keys[n * 4 * fp:]


def run_batch(lib, cid, fp, sizes, keys, msgs, sigs, allow_dups=0, want_gt=True):
    nb = len(sizes)
    verdicts = out(nb)
    gt = out(nb * 12 * fp) if want_gt else None
    rc = lib.bgls_verify_aggregate_batch(cid, B(b"".join(sigs)), B(keys), offs(sizes), nb, B(b"".join(msgs)), offs([len(m) for m in msgs]),
                                         allow_dups, verdicts, gt)
    return rc, list(verdicts)[:nb], (bytes(gt) if want_gt else None)


def single(lib, cid, fp, sig, keys, msgs, allow_dups=0):
    return lib.bgls_verify_aggregate(cid, B(sig), B(keys), B(b"".join(msgs)), offs([len(m) for m in msgs]), len(msgs), allow_dups)


def single_gt(lib, cid, fp, sig, keys, msgs):
    """the single path's GT element through a one-device key set (bgls_verify_aggregate_h_gt; the duplicate rule does not touch it)"""
    n = len(msgs)
    h = ctypes.c_uint64()
    devs = (ctypes.c_int * 1)(0)
    assert lib.bgls_keys_upload(cid, B(keys), n, devs, 1, 0, ctypes.byref(h)) == 0
    gt = out(12 * fp)
    rc = lib.bgls_verify_aggregate_h_gt(h, B(sig), B(b"".join(msgs)), offs([len(m) for m in msgs]), n, 1, gt)
    assert lib.bgls_keys_free(h) == 0
    assert rc in (0, 1)
    return bytes(gt)


SIZES = [0, 1, 2, 5, 6, 7, 59, 60, 61, 128, 129, 300, 1000]


def test_ragged_instances_match_single_calls(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    kinds = ["valid", "wrong_sig", "swap", "wrong_key", "dup"]
    plan = []
    for b, c in enumerate(SIZES):
        k = kinds[b % len(kinds)]
        if c < 2 and k in ("swap", "dup"):
            k = "valid"
        plan.append(k)
    plan[0] = "valid"                                    # the empty instance: sigma = infinity is accepted
    keys, msgs, sigs, spare = make_batch(lib, cid, fp, SIZES, 77 + cid, dup_in=[b for b, k in enumerate(plan) if k == "dup"])
    keys, sigs = bytearray(keys), list(sigs)
    at = 0
    for b, (c, k) in enumerate(zip(SIZES, plan)):
        if k == "wrong_sig":
            sigs[b] = sigs[(b + 1) % len(SIZES)] if SIZES[(b + 1) % len(SIZES)] else sigs[(b + 2) % len(SIZES)]
        elif k == "swap":
            msgs[at], msgs[at + c - 1] = msgs[at + c - 1], msgs[at]
        elif k == "wrong_key":
            keys[(at + c // 2) * 4 * fp:(at + c // 2 + 1) * 4 * fp] = spare
        at += c
    keys = bytes(keys)
    # one more instance without keys and with a signature that is not infinity: refused
    sizes = SIZES + [0]
    sigs.append(sigs[1])
    plan.append("empty_sig")
    rc, verdicts, gts = run_batch(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == sum(verdicts) and rc >= 0
    at = 0
    for b, c in enumerate(sizes):
        kb, mb = keys[at * 4 * fp:(at + c) * 4 * fp], msgs[at:at + c]
        want = single(lib, cid, fp, sigs[b], kb, mb)
        assert want in (0, 1)
        assert verdicts[b] == want, (b, c, plan[b])
        assert want == (1 if plan[b] == "valid" else 0), (b, c, plan[b])
        if c:
            assert gts[b * 12 * fp:(b + 1) * 12 * fp] == single_gt(lib, cid, fp, sigs[b], kb, mb), (b, c, plan[b])
        if 1 <= c <= 64:
            assert coracle.verify_aggregate(cid, sigs[b], kb, mb, False, threads=8) == want, (b, c, plan[b])
        at += c


def test_headline_sixteen_instances_of_2_16(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n1 = 1 << 16
    sizes = [n1] * 16
    keys, msgs, sigs, _ = make_batch(lib, cid, fp, sizes, 5 + cid, dup_in=[11])
    sigs[3] = sigs[4]                                    # a valid G1 point that is not instance 3's aggregate
    rc, verdicts, gts = run_batch(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == 14
    assert [b for b in range(16) if verdicts[b] != 1] == [3, 11]
    for b in (0, 9):
        kb, mb = keys[b * n1 * 4 * fp:(b + 1) * n1 * 4 * fp], msgs[b * n1:(b + 1) * n1]
        assert gts[b * 12 * fp:(b + 1) * 12 * fp] == single_gt(lib, cid, fp, sigs[b], kb, mb), b
    # instance 11 is a valid aggregate: only the duplicate rule refuses it
    rc, verdicts, _ = run_batch(lib, cid, fp, sizes, keys, msgs, sigs, allow_dups=1, want_gt=False)
    assert rc == 15 and verdicts[3] == 0 and verdicts[11] == 1


def test_one_scope_per_stage_for_the_whole_batch(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [200] * 16
    keys, msgs, sigs, _ = make_batch(lib, cid, fp, sizes, 31 + cid)

    def launches(stage):
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        assert lib.bgls_profile_get(stage.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0
        return cnt.value

    try:
        assert lib.bgls_profile_enable(1) == 0
        rc, verdicts, _ = run_batch(lib, cid, fp, sizes, keys, msgs, sigs, want_gt=False)
        assert rc == 16
        assert [launches(s) for s in ("h2c", "miller", "final_exp", "scatter", "epilogue")] == [1, 1, 1, 1, 1]
        assert lib.bgls_profile_enable(1) == 0
        for b in range(16):
            kb, mb = keys[b * 200 * 4 * fp:(b + 1) * 200 * 4 * fp], msgs[b * 200:(b + 1) * 200]
            assert single(lib, cid, fp, sigs[b], kb, mb) == 1
        assert [launches(s) for s in ("h2c", "miller", "final_exp")] == [16, 16, 16]
    finally:
        lib.bgls_profile_enable(0)


def test_duplicates_count_within_an_instance_only(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [3, 4, 5]
    keys, msgs, sigs, _ = make_batch(lib, cid, fp, sizes, 91 + cid, dup_in=[2])
    # instances 0 and 1 share one message: instance 1 re-signed with instance 0's first message at its position 2 (make_batch draws the
    # secret keys first from the same seed)
    msgs = list(msgs)
    msgs[3 + 2] = msgs[0]
    rnd = random.Random(91 + cid)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(sum(sizes) + 1)]
    kb = b"".join(s.to_bytes(32, "big") for s in sks[3:7])
    s1 = out(4 * 2 * fp)
    assert lib.bgls_sign_batch(cid, B(kb), B(b"".join(msgs[3:7])), offs([len(m) for m in msgs[3:7]]), 4, s1) == 0
    agg1 = out(2 * fp)
    assert lib.bgls_aggregate_points(cid, 1, s1, 4, agg1) == 0
    sigs = list(sigs)
    sigs[1] = bytes(agg1)
    rc, verdicts, _ = run_batch(lib, cid, fp, sizes, keys, msgs, sigs, want_gt=False)
    assert verdicts == [1, 1, 0] and rc == 2
    for b, lo, hi in ((0, 0, 3), (1, 3, 7), (2, 7, 12)):
        assert single(lib, cid, fp, sigs[b], keys[lo * 4 * fp:hi * 4 * fp], msgs[lo:hi]) == verdicts[b]
    rc, verdicts, _ = run_batch(lib, cid, fp, sizes, keys, msgs, sigs, allow_dups=1, want_gt=False)
    assert verdicts == [1, 1, 1] and rc == 3


def test_errors_forms_and_python_mirror(gpu_lib, curve):
    import torch
    from bgls_amd import Altbn128, Bls12, bgls
    from bgls_amd.curves import Point, G1, G2
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sizes = [7, 0, 130, 61]
    keys, msgs, sigs, _ = make_batch(lib, cid, fp, sizes, 13 + cid)
    sigs = list(sigs)
    sigs[1] = bytes(2 * fp)
    sigs[2] = sigs[3]
    nb = len(sizes)
    rc, verdicts, gts = run_batch(lib, cid, fp, sizes, keys, msgs, sigs)
    assert rc == 3 and verdicts == [1, 1, 0, 1]
    # an off-curve key anywhere fails the whole call
    bad = bytearray(keys)
    bad[(7 + 100) * 4 * fp:(7 + 101) * 4 * fp] = b"\xff" * (4 * fp)
    assert run_batch(lib, cid, fp, sizes, bytes(bad), msgs, sigs)[0] == ERR_ENCODING
    # offsets: not monotone, not from 0; an empty batch
    v = out(nb)
    moff = offs([len(m) for m in msgs])
    for io in ([0, 7, 5, 137, 198], [1, 7, 7, 137, 198]):
        arr = (ctypes.c_uint64 * 5)(*io)
        assert lib.bgls_verify_aggregate_batch(cid, B(b"".join(sigs)), B(keys), arr, nb, B(b"".join(msgs)), moff, 0, v, None) == ERR_ARG
    assert lib.bgls_verify_aggregate_batch(cid, None, None, offs([]), 0, None, offs([]), 0, None, None) == 0
    # the device form: same verdicts and GT bytes
    dev = torch.device("cuda:0")
    d_sigs = torch.tensor(list(b"".join(sigs)), dtype=torch.uint8, device=dev)
    d_keys = torch.tensor(list(keys), dtype=torch.uint8, device=dev)
    d_msgs = torch.tensor(list(b"".join(msgs)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    v2, gt2 = out(nb), out(nb * 12 * fp)
    rc2 = lib.bgls_verify_aggregate_batch_dev(cid, d_sigs.data_ptr(), d_keys.data_ptr(), offs(sizes), nb, d_msgs.data_ptr(), 32, 32, 0, v2, gt2, None)
    assert rc2 == 3 and list(v2)[:nb] == verdicts and bytes(gt2) == gts
    # the Python mirror equals the list of single calls
    cv = Altbn128 if cid == 0 else Bls12
    at, ks, ms = 0, [], []
    for c in sizes:
        ks.append([Point(cv, G2, keys[i * 4 * fp:(i + 1) * 4 * fp]) for i in range(at, at + c)])
        ms.append(msgs[at:at + c])
        at += c
    ps = [Point(cv, G1, s) for s in sigs]
    want = [bgls.VerifyAggregateSignature(cv, s, k, m) for s, k, m in zip(ps, ks, ms)]
    assert want == [True, True, False, True]
    assert bgls.VerifyAggregateSignatures(cv, ps, ks, ms) == want
    assert bgls.KoskVerifyAggregateSignatures(cv, ps, ks, ms) == [bgls.KoskVerifyAggregateSignature(cv, s, k, m) for s, k, m in zip(ps, ks, ms)]
