"""GPU tier: multi-signatures by signer bitmap against a resident key set (bgls_aggregate_subsets_h, bgls_verify_multi_subsets_h,
bgls_verify_multi_subsets_keys_dev).  Keys come from bgls_scale_generator, a set's signature is made with the sum of its signers'
secret keys through bgls_sign_batch.  Every case runs with bgls_set_subset_complement at 0, 1 and 2 and the three results must be
identical: the key sums against the C oracle byte for byte, the verifications against bgls_verify_multi_sets / bgls_aggregate_sets on
the gathered keys."""
import ctypes
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2
MODES = (0, 1, 2)


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offs(counts):
    o = (ctypes.c_uint64 * (len(counts) + 1))()
    for i, c in enumerate(counts):
        o[i + 1] = o[i] + c
    return o


def order(cid):
    from bgls_amd import Altbn128, Bls12
    return (Altbn128 if cid == 0 else Bls12).GetG1Order()


def upload(lib, cid, keys, n, devices=(0,), flags=0):
    h = ctypes.c_uint64()
    devs = (ctypes.c_int * len(devices))(*devices)
    rc = lib.bgls_keys_upload(cid, B(keys), n, devs, len(devices), flags, ctypes.byref(h))
    return rc, h.value


_SETS = {}


def key_set(lib, cid, fp, n, sks=None):
    """(secret keys, wire keys, handle) of an n-key set, made once per (curve, n) and shared by the tests"""
    tag = (cid, n) if sks is None else (cid, tuple(sks))
    if tag not in _SETS:
        if sks is None:
            rnd = random.Random(1000 * n + cid)
            sks = [rnd.randrange(1, 1 << 250) for _ in range(n)]
        keys = out(n * 4 * fp)
        assert lib.bgls_scale_generator(cid, 2, B(b"".join(s.to_bytes(32, "big") for s in sks)), n, keys) == 0
        rc, h = upload(lib, cid, bytes(keys), n)
        assert rc == 0
        _SETS[tag] = (list(sks), bytes(keys), h)
    return _SETS[tag]


def rows_of(n, subsets, stride=None):
    stride = (n + 7) // 8 if stride is None else stride
    rows = bytearray(stride * len(subsets))
    for b, sub in enumerate(subsets):
        for i in sub:
            rows[b * stride + (i >> 3)] |= 1 << (i & 7)
    return rows, stride


def gather(keys, fp, sub):
    return b"".join(keys[i * 4 * fp:(i + 1) * 4 * fp] for i in sorted(sub))


def sign_subsets(lib, cid, fp, sks, subsets, msgs):
    """signature b = (sum of the secret keys of subset b) H(msgs[b]); the point at infinity where that sum is 0 mod r"""
    r = order(cid)
    sums = [sum(sks[i] for i in sub) % r for sub in subsets]
    sigs = out(len(subsets) * 2 * fp)
    assert lib.bgls_sign_batch(cid, B(b"".join((s or 1).to_bytes(32, "big") for s in sums)), B(b"".join(msgs)), offs([len(m) for m in msgs]), len(subsets), sigs) == 0
    sigs = bytes(sigs)
    return [sigs[b * 2 * fp:(b + 1) * 2 * fp] if sums[b] else bytes(2 * fp) for b in range(len(subsets))]


def aggregate(lib, h, fp, n, subsets, stride=None):
    rows, stride = rows_of(n, subsets, stride)
    o = out(len(subsets) * 4 * fp)
    rc = lib.bgls_aggregate_subsets_h(h, B(rows), stride, len(subsets), o)
    return rc, bytes(o)


def in_every_mode(lib, fn):
    """fn() under bgls_set_subset_complement 0, 1 and 2: the three results are identical; returns one"""
    got = []
    try:
        for mode in MODES:
            assert lib.bgls_set_subset_complement(mode) == 0
            got.append(fn())
    finally:
        lib.bgls_set_subset_complement(0)
    assert got[1] == got[0] and got[2] == got[0], "the result depends on the complement mode"
    return got[0]


def verify_host(lib, h, fp, n, sigs, subsets, msgs, stride=None):
    nb = len(subsets)
    rows, stride = rows_of(n, subsets, stride)
    v, apk, gt = out(nb), out(nb * 4 * fp), out(nb * 12 * fp)
    rc = lib.bgls_verify_multi_subsets_h(h, B(b"".join(sigs)), B(rows), stride, nb, B(b"".join(msgs)), offs([len(m) for m in msgs]), v, apk, gt)
    return rc, list(v)[:nb], bytes(apk), bytes(gt)


def verify_dev(lib, h, fp, n, sigs, subsets, msgs, stride=None, raw_rows=None):
    """the device form: fixed-length messages, rows at a stride that is a multiple of 4"""
    import torch
    nb = len(subsets)
    stride = (n + 31) // 32 * 4 if stride is None else stride
    rows = raw_rows if raw_rows is not None else rows_of(n, subsets, stride)[0]
    L = len(msgs[0])
    assert all(len(m) == L for m in msgs)
    dev = torch.device("cuda:0")
    d_sigs = torch.tensor(list(b"".join(sigs)), dtype=torch.uint8, device=dev)
    d_rows = torch.tensor(list(bytes(rows) or b"\0\0\0\0"), dtype=torch.uint8, device=dev)
    d_msgs = torch.tensor(list(b"".join(msgs)), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    v, apk, gt = out(nb), out(nb * 4 * fp), out(nb * 12 * fp)
    rc = lib.bgls_verify_multi_subsets_keys_dev(h, d_sigs.data_ptr(), d_rows.data_ptr(), stride, nb, d_msgs.data_ptr(), L, L, v, apk, gt, None)
    return rc, list(v)[:nb], bytes(apk), bytes(gt)


def gathered_reference(lib, cid, fp, keys, sigs, subsets, msgs):
    """bgls_verify_multi_sets and bgls_aggregate_sets on the gathered keys: (rc, verdicts, key sums, GT elements)"""
    nb = len(subsets)
    flat = b"".join(gather(keys, fp, sub) for sub in subsets)
    sizes = [len(set(sub)) for sub in subsets]
    v, gt, apk = out(nb), out(nb * 12 * fp), out(nb * 4 * fp)
    rc = lib.bgls_verify_multi_sets(cid, B(b"".join(sigs)), B(flat), offs(sizes), nb, B(b"".join(msgs)), offs([len(m) for m in msgs]), v, gt)
    assert lib.bgls_aggregate_sets(cid, 2, B(flat), offs(sizes), nb, apk) == 0
    return rc, list(v)[:nb], bytes(apk), bytes(gt)


def row_shapes(n, seed):
    """about a dozen rows: empty, one bit first / last, all ones, exactly n / 2 and n / 2 + 1 selected (the two sides of the mode rule),
    all but one, random at 10 % and 90 %"""
    rnd = random.Random(seed)
    everyone = list(range(n))
    half = rnd.sample(everyone, n // 2)
    rest = [i for i in everyone if i not in set(half)]
    return [[], [0], [n - 1], everyone, half, half + rest[:1], everyone[1:], everyone[:-1], [i for i in everyone if i != n // 2],
            [i for i in everyone if rnd.random() < 0.1], [i for i in everyone if rnd.random() < 0.9], [i for i in everyone if rnd.random() < 0.5]]


@pytest.mark.parametrize("n", [1, 33, 65, 2049, 4100])
def test_aggregate_subsets_against_the_c_oracle(gpu_lib, curve, n):
    """4100 keys: three windows and more than one block per set"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    sks, keys, h = key_set(lib, cid, fp, n)
    subsets = row_shapes(n, n + cid)
    want = b"".join(coracle.aggregate_points(cid, 2, gather(keys, fp, sub), len(sub)) for sub in subsets)
    rc, got = in_every_mode(lib, lambda: aggregate(lib, h, fp, n, subsets))
    assert rc == 0
    for b, sub in enumerate(subsets):
        assert got[b * 4 * fp:(b + 1) * 4 * fp] == want[b * 4 * fp:(b + 1) * 4 * fp], (b, len(sub))
    # a wider stride (padding bytes zero) changes nothing
    assert aggregate(lib, h, fp, n, subsets, stride=(n + 7) // 8 + 5) == (0, want)


def test_exceptional_points(gpu_lib, curve):
    """Every answer comes from the oracle.  The set holds K, -K (secret r - k), K a second time and -- where an unchecked upload admits
    it -- a key at infinity."""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    r = order(cid)
    k = 0x1234567890ABCDEF1234567
    sks3, keys3, h3 = key_set(lib, cid, fp, 3, sks=[k, r - k, k])
    assert coracle.aggregate_points(cid, 2, keys3[:2 * 4 * fp], 2) == bytes(4 * fp), "K + (-K) is not infinity: the fixture is wrong"
    rc4, h4 = upload(lib, cid, keys3 + bytes(4 * fp), 4)
    sets = [(h3, keys3, 3, sks3)] + ([(h4, keys3 + bytes(4 * fp), 4, sks3 + [0])] if rc4 == 0 else [])
    msg = b"exceptional"
    for h, keys, n, sks in sets:
        subsets = [s for s in ([0, 1], [0, 2], [0, 1, 2], [1, 2], [1], [], [3], [0, 1, 3], [0, 1, 2, 3], [2, 3]) if all(i < n for i in s)]
        want = b"".join(coracle.aggregate_points(cid, 2, gather(keys, fp, sub), len(sub)) for sub in subsets)
        assert want[:4 * fp] == bytes(4 * fp)                     # {K, -K}: a subset summing to infinity
        # n = 3, {K, -K} selected: 2 * 2 > 3 chooses the complement, and -K + (K - K + K) is infinity
        assert in_every_mode(lib, lambda: aggregate(lib, h, fp, n, subsets)) == (0, want)
        # the verdict of a subset summing to infinity is 1 only for the infinity signature
        sigs = sign_subsets(lib, cid, fp, sks, subsets, [msg] * len(subsets))
        assert sigs[0] == bytes(2 * fp)
        other = sigs[1]
        for form in (verify_host, verify_dev):
            rc, v, apk, gt = in_every_mode(lib, lambda: form(lib, h, fp, n, sigs, subsets, [msg] * len(subsets)))
            assert rc == len(subsets) and v == [1] * len(subsets) and apk == want
            rc, v, _, _ = in_every_mode(lib, lambda: form(lib, h, fp, n, [other] + sigs[1:], subsets, [msg] * len(subsets)))
            assert rc == len(subsets) - 1 and v == [0] + [1] * (len(subsets) - 1)
        for b, sub in enumerate(subsets):
            assert coracle.verify_multi(cid, sigs[b], gather(keys, fp, sub), len(sub), msg) == 1, b
    if rc4 == 0:
        assert lib.bgls_keys_free(h4) == 0


def test_the_doubling_branch_of_the_mixed_addition(gpu_lib, curve):
    """67 keys: key 0 and key 32 are the two copies of K, the other 65 are distinct random keys.  Row 0 selects keys 0 .. 32: 33 entries
    in one compaction step, so lane pair 0 takes entry 0 (K) in the first round of 32 and entry 32 (K again) in the second -- its
    accumulator is K alone when the copy arrives, whatever the 31 keys between them are (they go to pairs 1 .. 31): any 31 distinct keys
    serve.  Row 1 selects everything else, so with the complement forced the same 33 entries arrive negated (-K meets -K).  Row 2 is the
    two copies alone: they meet in the block tree instead."""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    rnd = random.Random(67 + cid)
    k = rnd.randrange(1, 1 << 250)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(67)]
    sks[0] = sks[32] = k
    sks, keys, h = key_set(lib, cid, fp, 67, sks=sks)
    subsets = [list(range(33)), list(range(33, 67)), [0, 32], list(range(67))]
    want = b"".join(coracle.aggregate_points(cid, 2, gather(keys, fp, sub), len(sub)) for sub in subsets)
    assert in_every_mode(lib, lambda: aggregate(lib, h, fp, 67, subsets)) == (0, want)


def test_verify_against_verify_multi_sets(gpu_lib, curve):
    """twelve sets over a 2049-key set: nine valid, one with a bit flipped in its row, one with a changed message, one with the signature
    of another set; host and device forms against bgls_verify_multi_sets / bgls_aggregate_sets on the gathered keys"""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 2049
    sks, keys, h = key_set(lib, cid, fp, n)
    rnd = random.Random(12 + cid)
    subsets = row_shapes(n, 99 + cid)[1:]
    subsets.append(rnd.sample(range(n), 700))
    assert len(subsets) == 12
    msgs = [rnd.randbytes(32) for _ in subsets]
    sigs = sign_subsets(lib, cid, fp, sks, subsets, msgs)
    subsets[3] = [i for i in subsets[3] if i != 1000] if 1000 in subsets[3] else subsets[3] + [1000]      # a flipped bit
    msgs[6] = bytes([msgs[6][0] ^ 1]) + msgs[6][1:]                                                      # a changed message
    sigs[9] = sigs[8]                                                                                    # another set's signature
    want = gathered_reference(lib, cid, fp, keys, sigs, subsets, msgs)
    assert want[0] == 9 and want[1] == [0 if b in (3, 6, 9) else 1 for b in range(12)]
    assert in_every_mode(lib, lambda: verify_host(lib, h, fp, n, sigs, subsets, msgs)) == want
    assert in_every_mode(lib, lambda: verify_dev(lib, h, fp, n, sigs, subsets, msgs)) == want
    # nullable outputs
    rows, stride = rows_of(n, subsets)
    v = out(12)
    assert lib.bgls_verify_multi_subsets_h(h, B(b"".join(sigs)), B(rows), stride, 12, B(b"".join(msgs)), offs([32] * 12), v, None, None) == 9
    assert list(v)[:12] == want[1]


def test_small_sets_against_the_oracle_pairing(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 65
    sks, keys, h = key_set(lib, cid, fp, n)
    subsets = [[0], [64], list(range(65)), list(range(0, 65, 2)), []]
    msgs = [b"m%d" % b * 4 for b in range(5)]
    sigs = sign_subsets(lib, cid, fp, sks, subsets, msgs)
    sigs[3] = sigs[2]
    sigs[4] = sigs[0]
    oracle = [coracle.verify_multi(cid, sigs[b], gather(keys, fp, subsets[b]), len(subsets[b]), msgs[b]) for b in range(5)]
    assert oracle == [1, 1, 1, 0, 0]                              # the empty subset with a signature that is not infinity is refused
    for form in (verify_host, verify_dev):
        rc, v, apk, gt = in_every_mode(lib, lambda: form(lib, h, fp, n, sigs, subsets, msgs))
        assert rc == 3 and v == oracle
        assert apk == b"".join(coracle.aggregate_points(cid, 2, gather(keys, fp, s), len(s)) for s in subsets)
    sigs[4] = bytes(2 * fp)                                       # ... and accepted with the infinity signature
    assert in_every_mode(lib, lambda: verify_host(lib, h, fp, n, sigs, subsets, msgs))[1] == [1, 1, 1, 0, 1]


def test_status_and_errors(gpu_lib, curve):
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    n = 65
    sks, keys, h = key_set(lib, cid, fp, n)
    subsets = [[0, 5, 64], list(range(40)), [7]]
    msgs = [bytes([b]) * 16 for b in range(3)]
    sigs = sign_subsets(lib, cid, fp, sks, subsets, msgs)
    good = verify_dev(lib, h, fp, n, sigs, subsets, msgs)
    assert good[0] == 3
    # a stray bit beyond n: found on the host by the host forms, by the planning pass of the device form; the next valid call is right
    stride = 12
    for stray in (65, 70, 95):
        rows, _ = rows_of(n, subsets, stride)
        rows[stride + (stray >> 3)] |= 1 << (stray & 7)
        assert in_every_mode(lib, lambda: verify_dev(lib, h, fp, n, sigs, subsets, msgs, stride=stride, raw_rows=rows)[0]) == ERR_ARG
        assert verify_dev(lib, h, fp, n, sigs, subsets, msgs) == good
        v = out(3)
        assert lib.bgls_verify_multi_subsets_h(h, B(b"".join(sigs)), B(rows), stride, 3, B(b"".join(msgs)), offs([16] * 3), v, None, None) == ERR_ARG
        assert lib.bgls_aggregate_subsets_h(h, B(rows), stride, 3, out(3 * 4 * fp)) == ERR_ARG
    assert verify_host(lib, h, fp, n, sigs, subsets, msgs) == good
    # stride below ceil(n / 8); an unknown handle
    assert verify_host(lib, h, fp, n, sigs, subsets, msgs, stride=8)[0] == ERR_ARG
    assert verify_dev(lib, h, fp, n, sigs, subsets, msgs, stride=8)[0] == ERR_ARG
    assert aggregate(lib, h, fp, n, subsets, stride=8)[0] == ERR_ARG
    assert verify_host(lib, 0xDEADBEEF, fp, n, sigs, subsets, msgs)[0] == ERR_ARG
    assert aggregate(lib, 0xDEADBEEF, fp, n, subsets)[0] == ERR_ARG
    # an off-curve signature anywhere fails the whole call
    bad = [sigs[0], bytes(2 * fp - 1) + b"\x01", sigs[2]]
    assert in_every_mode(lib, lambda: verify_host(lib, h, fp, n, bad, subsets, msgs)[0]) == ERR_ENCODING
    assert verify_dev(lib, h, fp, n, bad, subsets, msgs)[0] == ERR_ENCODING
    assert verify_host(lib, h, fp, n, sigs, subsets, msgs) == good
    # a two-shard set is refused
    rc, h2 = upload(lib, cid, keys, n, devices=(0, 0))
    assert rc == 0
    try:
        assert verify_host(lib, h2, fp, n, sigs, subsets, msgs)[0] == ERR_ARG
        assert verify_dev(lib, h2, fp, n, sigs, subsets, msgs)[0] == ERR_ARG
        assert aggregate(lib, h2, fp, n, subsets)[0] == ERR_ARG
    finally:
        assert lib.bgls_keys_free(h2) == 0


def test_python_mirrors(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    from bgls_amd.curves import Point, G1, G2
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    cv = Altbn128 if cid == 0 else Bls12
    n = 33
    sks, keys, _ = key_set(lib, cid, fp, n)
    ks = bgls.KeySet(cv, [Point(cv, G2, keys[i * 4 * fp:(i + 1) * 4 * fp]) for i in range(n)])
    subsets = [[0, 1, 32], list(range(33)), [], [5]]
    msgs = [b"alpha", b"beta", b"gamma", b"delta"]
    bitmaps = [bytes(rows_of(n, [s])[0]) for s in subsets]
    want_keys = [coracle.aggregate_points(cid, 2, gather(keys, fp, s), len(s)) for s in subsets]
    assert [p.raw for p in bgls.AggregateKeysBySubset(ks, subsets)] == want_keys
    assert [p.raw for p in bgls.AggregateKeysBySubset(ks, bitmaps)] == want_keys
    assert bgls.AggregateKeysBySubset(ks, []) == []
    for kosk in (False, True):
        signed = [b"\x01" + m for m in msgs] if kosk else msgs
        sigs = [Point(cv, G1, s) for s in sign_subsets(lib, cid, fp, sks, subsets, signed)]
        sigs[3] = sigs[0]
        fn = bgls.KoskVerifyMultiSignaturesBySubset if kosk else bgls.VerifyMultiSignaturesBySubset
        got = fn(cv, sigs, ks, subsets, msgs)
        assert got == [True, True, True, False]
        assert fn(cv, sigs, ks, bitmaps, msgs) == got                     # index lists and bitmaps give the same result
        assert bgls.VerifyMultiSignaturesBySubset(cv, sigs, ks, subsets, signed) == got      # the Kosk form equals the plain form on prefixed messages
        single = bgls.KoskVerifyMultiSignature if kosk else bgls._verify_multi
        assert got == [single(cv, s, [Point(cv, G2, keys[i * 4 * fp:(i + 1) * 4 * fp]) for i in sub], m) for s, sub, m in zip(sigs, subsets, msgs)]
    # a nil signature is False alone; an index outside the set is the caller's error
    assert bgls.VerifyMultiSignaturesBySubset(cv, [None] + sigs[1:], ks, subsets, [b"\x01" + m for m in msgs])[0] is False
    with pytest.raises(ValueError):
        bgls.AggregateKeysBySubset(ks, [[33]])
    ks.free()
