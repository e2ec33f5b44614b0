"""GPU tier: the distinct-message defence (bgls/blsDistinctMessage.go) and the key-possession check (bgls/blsKosk.go:59-69) with their hash
inputs built on the device from keys that are already there (k_keymsgs.hip).

The yardstick everywhere is the library's own older path: the existing calls, fed messages that this file prefixes on the host (key wire
bytes || message for the distinct-message calls, the output of bgls_compress_points for the proofs of possession).  The C oracle is the
second witness for verdicts.  Valid signatures are made with bgls_scale_generator and bgls_sign_batch on the host-prefixed messages."""
import ctypes
import random

import pytest

from oracle import coracle

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_ENCODING = -1, -2
ORDER = {0: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
         1: 52435875175126190479447740508185965837690552500527637822603658699938581184513}
# message lengths of the ragged cases: the issue's set, and the lengths that end a hash input exactly on, one below and one above a hash
# block -- 8 +- 1 behind a 128-byte alt-bn128 key (Keccak rate 136), 64 +- 1 behind a 192-byte BLS12-381 key (BLAKE2b block 128)
LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65]
POOL = 140


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def out(n):
    return (ctypes.c_uint8 * max(1, n))()


def offsets(msgs, first=0):
    off = (ctypes.c_uint64 * (len(msgs) + 1))()
    acc = first
    for i, m in enumerate(msgs):
        off[i] = acc
        acc += len(m)
    off[len(msgs)] = acc
    return off


def cut(raw, size):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


def ragged(rnd, n, shift=0):
    return [rnd.randbytes(LENGTHS[(7 * i + shift) % len(LENGTHS)]) for i in range(n)]


class Pool:
    """POOL key pairs of one curve, made once; signatures on any messages under any of them"""

    def __init__(self, lib, cid, fp):
        self.lib, self.cid, self.fp = lib, cid, fp
        self.G1B, self.G2B, self.GTB = 2 * fp, 4 * fp, 12 * fp
        rnd = random.Random(4242 + cid)
        self.sks = [rnd.randrange(1, ORDER[cid]).to_bytes(32, "big") for _ in range(POOL)]
        kbuf = out(POOL * self.G2B)
        assert lib.bgls_scale_generator(cid, 2, B(b"".join(self.sks)), POOL, kbuf) == 0
        self.keys = cut(bytes(kbuf), self.G2B)
        cbuf = out(POOL * self.G2B // 2)
        assert lib.bgls_compress_points(cid, 2, kbuf, POOL, cbuf) == 0
        self.compressed = cut(bytes(cbuf), self.G2B // 2)

    def sign(self, idx, msgs):
        """signatures of the keys idx on msgs, taken as they are (already prefixed or not)"""
        n = len(idx)
        sg = out(n * self.G1B)
        if n:
            assert self.lib.bgls_sign_batch(self.cid, B(b"".join(self.sks[i] for i in idx)), B(b"".join(msgs)), offsets(msgs), n, sg) == 0
        return cut(bytes(sg), self.G1B)[:n]

    def sign_distinct(self, idx, msgs):
        return self.sign(idx, [self.keys[i] + m for i, m in zip(idx, msgs)])

    def aggregate(self, sigs):
        ag = out(self.G1B)
        assert self.lib.bgls_aggregate_points(self.cid, 1, B(b"".join(sigs)), len(sigs), ag) == 0
        return bytes(ag)


_pools = {}


@pytest.fixture
def pool(gpu_lib, curve):
    if curve["id"] not in _pools:
        _pools[curve["id"]] = Pool(gpu_lib, curve["id"], curve["fp"])
    return _pools[curve["id"]]


def hash_host(p, msgs):
    o = out(len(msgs) * p.G1B)
    assert p.lib.bgls_hash_to_g1(p.cid, B(b"".join(msgs)), offsets(msgs), len(msgs), o) == 0
    return bytes(o)


def hash_keyed(p, mode, keys, msgs=None, first=0):
    n = len(keys)
    o = out(n * p.G1B)
    blob, off = (None, None) if msgs is None else (B(bytes(first) + b"".join(msgs)), offsets(msgs, first))
    assert p.lib.bgls_hash_to_g1_keyed(p.cid, mode, B(b"".join(keys)), blob, off, n, o) == 0
    return bytes(o)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_built_bytes(pool, n):
    """mode 0: the hash of key || message, byte for byte, on both sides of the kernel's wave (4 inputs) and block (16 inputs) boundaries, for
    ragged, empty and equal-length messages and a blob that does not start at offset 0; mode 1: the hash of the compressed keys"""
    p, rnd = pool, random.Random(100 + n)
    keys = p.keys[:n]
    for msgs, first in ((ragged(rnd, n, n), 0), (ragged(rnd, n, 3), 5), ([b""] * n, 0), ([rnd.randbytes(32) for _ in range(n)], 0),
                        ([rnd.randbytes(9) for _ in range(n)], 3)):
        assert hash_keyed(p, 0, keys, msgs, first) == hash_host(p, [k + m for k, m in zip(keys, msgs)]), ([len(m) for m in msgs], first)
    assert hash_keyed(p, 1, keys) == hash_host(p, p.compressed[:n])


def test_block_boundary_lengths(pool):
    """every length of LENGTHS behind every alignment the previous inputs leave: the ragged batch above walks them in one order, this one
    puts each length behind each other length"""
    p, rnd = pool, random.Random(7)
    lens = [a for a in LENGTHS for _ in (0, 1)]
    rnd.shuffle(lens)
    msgs = [rnd.randbytes(L) for L in lens] + [rnd.randbytes(L) for L in (7, 8, 9, 63, 64, 65)]
    keys = p.keys[:len(msgs)]
    assert hash_keyed(p, 0, keys, msgs) == hash_host(p, [k + m for k, m in zip(keys, msgs)])


def distinct_cases(p, n, seed):
    """(name, aggregate signature, keys, payloads, expected verdict) around one valid n-signer instance"""
    rnd = random.Random(seed)
    idx = list(range(n))
    msgs = [rnd.randbytes(1 + LENGTHS[(5 * i) % len(LENGTHS)]) for i in range(n)]
    keys = [p.keys[i] for i in idx]
    agg = p.aggregate(p.sign_distinct(idx, msgs))
    cases = [("valid", agg, keys, msgs, 1)]
    j = n // 2
    flipped = list(msgs)
    flipped[j] = bytes([flipped[j][0] ^ 0x20]) + flipped[j][1:]
    cases.append(("message byte flipped", agg, keys, flipped, 0))
    other = list(keys)
    other[j] = p.keys[POOL - 1]
    cases.append(("key swapped for another valid key", agg, other, msgs, 0))
    if n >= 2:
        swapped = list(keys)
        swapped[0], swapped[n - 1] = swapped[n - 1], swapped[0]
        cases.append(("two keys exchanged", agg, swapped, msgs, 0))
    cases.append(("signed the plain way", p.aggregate(p.sign(idx, msgs)), keys, msgs, 0))
    same = [b"one payload for everybody"] * n
    cases.append(("identical payloads", p.aggregate(p.sign_distinct(idx, same)), keys, same, 1))
    twice_idx, twice_msgs = idx + [0], msgs + [msgs[0]]
    cases.append(("the same key and payload twice", p.aggregate(p.sign_distinct(twice_idx, twice_msgs)), keys + [keys[0]], twice_msgs, 1))
    return cases


@pytest.mark.parametrize("n", [1, 7, 65])
def test_aggregate_wire_keys(pool, n):
    p = pool
    for name, agg, keys, msgs, want in distinct_cases(p, n, 300 + n):
        pre = [k + m for k, m in zip(keys, msgs)]
        ref = p.lib.bgls_verify_aggregate(p.cid, B(agg), B(b"".join(keys)), B(b"".join(pre)), offsets(pre), len(keys), 1)
        got = p.lib.bgls_verify_aggregate_distinct(p.cid, B(agg), B(b"".join(keys)), B(b"".join(msgs)), offsets(msgs), len(keys))
        assert got == ref == want, (name, got, ref)
        if n == 7:
            assert coracle.verify_aggregate(p.cid, agg, b"".join(keys), pre, True, threads=8) == want, name


def devs(k):
    return (ctypes.c_int * k)(*([0] * k))


@pytest.mark.parametrize("prepare", [0, 2], ids=["plain", "prepared"])
@pytest.mark.parametrize("shards", [1, 2, 3])
def test_key_sets(pool, shards, prepare):
    """the cases of the wire-key test at n = 65 against key sets of 1, 2 and 3 shards on one device: verdict and GT bytes of
    bgls_verify_aggregate_h_gt on host-prefixed messages"""
    p = pool
    for name, agg, keys, msgs, want in distinct_cases(p, 65, 365):
        n = len(keys)
        h = ctypes.c_uint64()
        assert p.lib.bgls_keys_upload(p.cid, B(b"".join(keys)), n, devs(shards), shards, 1 | prepare, ctypes.byref(h)) == 0, name
        try:
            pre = [k + m for k, m in zip(keys, msgs)]
            gt_ref, gt = out(p.GTB), out(p.GTB)
            ref = p.lib.bgls_verify_aggregate_h_gt(h, B(agg), B(b"".join(pre)), offsets(pre), n, 1, gt_ref)
            got = p.lib.bgls_verify_aggregate_distinct_h(h, B(agg), B(b"".join(msgs)), offsets(msgs), n, gt)
            assert got == ref == want, (name, got, ref)
            assert bytes(gt) == bytes(gt_ref), name
            assert p.lib.bgls_verify_aggregate_distinct_h(h, B(agg), B(b"".join(msgs)), offsets(msgs), n, None) == want, name
            if name == "valid":
                assert p.lib.bgls_verify_aggregate_distinct_h(h, B(agg), B(b"".join(msgs)), offsets(msgs[:-1]), n - 1, None) == ERR_ARG
                assert p.lib.bgls_verify_aggregate_distinct_h(h, B(agg), B(b"".join(msgs + [b"x"])), offsets(msgs + [b"x"]), n + 1, None) == ERR_ARG
        finally:
            assert p.lib.bgls_keys_free(h) == 0


def dev_bytes(torch, data):
    return torch.tensor(list(data or b"\0"), dtype=torch.uint8, device=torch.device("cuda:0"))


SIZES = [0, 1, 2, 60, 61, 5]      # an empty instance, and instances that end on and one past the 60-pair Miller tile


def batch_instance(p, rnd, equal_len):
    """six instances of SIZES; instance 4 is tampered, the empty instance 0 has a signature that is not the point at infinity"""
    ioff, keys, msgs, sigs = [0], [], [], []
    for size in SIZES:
        idx = list(range(ioff[-1], ioff[-1] + size))
        ms = [rnd.randbytes(24) for _ in idx] if equal_len else ragged(rnd, size, len(keys))
        sigs.append(p.aggregate(p.sign_distinct(idx, ms)) if size else p.sign([3], [b"not infinity"])[0])
        keys += [p.keys[i] for i in idx]
        msgs += ms
        ioff.append(ioff[-1] + size)
    t = ioff[4] + 17
    msgs[t] = msgs[t][:-1] + bytes([msgs[t][-1] ^ 1]) if msgs[t] else b"\x01"
    return ioff, keys, msgs, sigs


def run_batch(p, fn, ioff, keys, msgs, sigs, *dups):
    n_inst = len(sigs)
    v, gt = out(n_inst), out(n_inst * p.GTB)
    rc = fn(p.cid, B(b"".join(sigs)), B(b"".join(keys)), (ctypes.c_uint64 * len(ioff))(*ioff), n_inst, B(b"".join(msgs)), offsets(msgs), *dups, v, gt)
    return rc, list(v)[:n_inst], bytes(gt)


@pytest.mark.parametrize("equal_len", [False, True], ids=["ragged", "fixed"])
def test_batch(pool, equal_len):
    import torch
    p = pool
    ioff, keys, msgs, sigs = batch_instance(p, random.Random(61 + p.cid), equal_len)
    pre = [k + m for k, m in zip(keys, msgs)]
    ref = run_batch(p, p.lib.bgls_verify_aggregate_batch, ioff, keys, pre, sigs, 1)
    got = run_batch(p, p.lib.bgls_verify_aggregate_distinct_batch, ioff, keys, msgs, sigs)
    assert ref[0] == 4 and ref[1] == [0, 1, 1, 1, 0, 1]
    assert got == ref
    if equal_len:
        bufs = [dev_bytes(torch, b"".join(sigs)), dev_bytes(torch, b"".join(keys)), dev_bytes(torch, b"".join(msgs))]
        torch.cuda.synchronize()
        v, gt = out(len(sigs)), out(len(sigs) * p.GTB)
        rc = p.lib.bgls_verify_aggregate_distinct_batch_dev(p.cid, bufs[0].data_ptr(), bufs[1].data_ptr(), (ctypes.c_uint64 * len(ioff))(*ioff), len(sigs),
                                                            bufs[2].data_ptr(), 24, 24, v, gt, None)
        assert (rc, list(v), bytes(gt)) == ref
    # an off-curve key fails the whole call, as it fails the sibling
    bad = list(keys)
    bad[70] = bad[70][:-1] + bytes([bad[70][-1] ^ 1])
    assert run_batch(p, p.lib.bgls_verify_aggregate_batch, ioff, bad, [k + m for k, m in zip(bad, msgs)], sigs, 1)[0] == ERR_ENCODING
    assert run_batch(p, p.lib.bgls_verify_aggregate_distinct_batch, ioff, bad, msgs, sigs)[0] == ERR_ENCODING


def run_sets(p, sigs, keys, hash_inputs):
    n = len(sigs)
    v, gt = out(n), out(n * p.GTB)
    rc = p.lib.bgls_verify_multi_sets(p.cid, B(b"".join(sigs)), B(b"".join(keys)), (ctypes.c_uint64 * (n + 1))(*range(n + 1)), n, B(b"".join(hash_inputs)),
                                      offsets(hash_inputs), v, gt)
    return rc, list(v), bytes(gt)


def test_single_batch(pool):
    """n = 9 DistinctMsgVerifySingleSignature calls, items 2 (a wrong key) and 7 (a wrong signature) bad: verdicts and GT bytes of
    bgls_verify_multi_sets on one-key sets with host-built messages; ragged and equal-length messages, and the device-buffer form"""
    import torch
    p, n = pool, 9
    rnd = random.Random(99 + p.cid)
    for equal_len in (False, True):
        idx = list(range(20, 20 + n))
        msgs = [rnd.randbytes(20) for _ in idx] if equal_len else ragged(rnd, n, 2)
        sigs = p.sign_distinct(idx, msgs)
        keys = [p.keys[i] for i in idx]
        keys[2] = p.keys[100]
        sigs[7] = sigs[6]
        ref = run_sets(p, sigs, keys, [k + m for k, m in zip(keys, msgs)])
        assert ref[0] == 7 and ref[1] == [1, 1, 0, 1, 1, 1, 1, 0, 1]
        v, gt = out(n), out(n * p.GTB)
        rc = p.lib.bgls_verify_single_distinct_batch(p.cid, B(b"".join(sigs)), B(b"".join(keys)), B(b"".join(msgs)), offsets(msgs), n, v, gt)
        assert (rc, list(v), bytes(gt)) == ref
        if equal_len:
            bufs = [dev_bytes(torch, b"".join(sigs)), dev_bytes(torch, b"".join(keys)), dev_bytes(torch, b"".join(msgs))]
            torch.cuda.synchronize()
            v, gt = out(n), out(n * p.GTB)
            rc = p.lib.bgls_verify_single_distinct_batch_dev(p.cid, bufs[0].data_ptr(), bufs[1].data_ptr(), n, bufs[2].data_ptr(), 20, 20, v, gt, None)
            assert (rc, list(v), bytes(gt)) == ref


def test_authentication_batch(pool):
    """n = 9 CheckAuthentication calls: the messages are the compressed keys, the valid items Authenticate's output"""
    p, n = pool, 9
    idx = list(range(40, 40 + n))
    auths = p.sign(idx, [p.compressed[i] for i in idx])
    keys = [p.keys[i] for i in idx]
    keys[2] = p.keys[101]
    auths[7] = auths[5]
    cbuf = out(n * p.G2B // 2)
    assert p.lib.bgls_compress_points(p.cid, 2, B(b"".join(keys)), n, cbuf) == 0
    ref = run_sets(p, auths, keys, cut(bytes(cbuf), p.G2B // 2))
    assert ref[0] == 7 and ref[1] == [1, 1, 0, 1, 1, 1, 1, 0, 1]
    v, gt = out(n), out(n * p.GTB)
    rc = p.lib.bgls_check_authentication_batch(p.cid, B(b"".join(keys)), B(b"".join(auths)), n, v, gt)
    assert (rc, list(v), bytes(gt)) == ref
    # second witness for one accepted and one rejected item
    for b in (0, 2):
        assert coracle.verify_multi(p.cid, auths[b], keys[b], 1, bytes(cbuf)[b * p.G2B // 2:(b + 1) * p.G2B // 2]) == ref[1][b]


def test_python_mirror(gpu_lib, curve):
    from bgls_amd import Altbn128, Bls12, bgls
    cv, foreign = (Altbn128, Bls12) if curve["id"] == 0 else (Bls12, Altbn128)
    rnd = random.Random(17 + curve["id"])
    n = 12
    sks = [rnd.randrange(1, ORDER[curve["id"]]) for _ in range(n)]
    keys = bgls.LoadPublicKeys(cv, sks)
    msgs = [rnd.randbytes(5 + i) for i in range(n)]
    sigs = bgls.SignBatch(cv, sks, [k.MarshalUncompressed() + m for k, m in zip(keys, msgs)])
    assert sigs[0].raw == bgls.DistinctMsgSign(cv, sks[0], msgs[0]).raw
    assert [h.raw for h in cv.HashToG1Keyed(keys[:3], msgs[:3])] == [cv.HashToG1(k.MarshalUncompressed() + m).raw for k, m in zip(keys[:3], msgs[:3])]
    assert [h.raw for h in cv.HashToG1Keyed(keys[:3])] == [cv.HashToG1(k.Marshal()).raw for k in keys[:3]]
    agg = bgls.AggregateSignatures(sigs)
    # a key set is accepted where the list of keys is
    ks = bgls.KeySet(cv, keys)
    try:
        assert bgls.DistinctMsgVerifyAggregateSignature(cv, agg, ks, msgs) is True
        assert bgls.DistinctMsgVerifyAggregateSignature(cv, agg, ks, msgs[:-1] + [b"tampered"]) is False
        assert bgls.DistinctMsgVerifyAggregateSignature(cv, agg, ks, msgs[:-1]) is False
    finally:
        ks.free()
    assert bgls.DistinctMsgVerifyAggregateSignature(cv, agg, keys, msgs) is True
    assert bgls.DistinctMsgVerifyAggregateSignature(cv, agg, keys[::-1], msgs) is False
    # the batch functions against the lists of single calls, on a mixed batch with a foreign-curve point and a length mismatch
    agg3, agg4 = bgls.AggregateSignatures(sigs[:3]), bgls.AggregateSignatures(sigs[3:7])
    inst_sigs = [agg3, agg4, agg4, foreign.GetG1(), agg3, agg3]
    inst_keys = [keys[:3], keys[3:7], keys[3:7], keys[:3], keys[:3], [foreign.GetG2()] + keys[1:3]]
    inst_msgs = [msgs[:3], msgs[3:7], msgs[3:6] + [b"other"], msgs[:3], msgs[:2], msgs[:3]]
    singles = [bgls.DistinctMsgVerifyAggregateSignature(cv, s, k, m) for s, k, m in zip(inst_sigs, inst_keys, inst_msgs)]
    assert singles == [True, True, False, False, False, False]
    assert bgls.DistinctMsgVerifyAggregateSignatures(cv, inst_sigs, inst_keys, inst_msgs) == singles
    one_sigs = sigs[:4] + [sigs[0], foreign.GetG1(), sigs[6]]
    one_keys = keys[:4] + [keys[4], keys[5], foreign.GetG2()]
    one_msgs = msgs[:3] + [b"other"] + msgs[4:7]
    singles = [bgls.DistinctMsgVerifySingleSignature(cv, s, k, m) for s, k, m in zip(one_sigs, one_keys, one_msgs)]
    assert singles == [True, True, True, False, False, False, False]
    assert bgls.DistinctMsgVerifySingleSignatures(cv, one_sigs, one_keys, one_msgs) == singles
    auths = [bgls.Authenticate(cv, sk) for sk in sks[:3]] + [sigs[3], foreign.GetG1()]
    singles = [bgls.CheckAuthentication(cv, k, a) for k, a in zip(keys[:5], auths)]
    assert singles == [True, True, True, False, False]
    assert bgls.CheckAuthentications(cv, keys[:5], auths) == singles


def test_profile_scope(pool):
    """a distinct call reports its gather under key_msgs and never runs the duplicate scan"""
    p, n = pool, 7
    _, agg, keys, msgs, _ = distinct_cases(p, n, 5)[0]

    def launches(stage):
        ms, cnt = ctypes.c_double(), ctypes.c_ulonglong()
        assert p.lib.bgls_profile_get(stage.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0
        return cnt.value

    try:
        assert p.lib.bgls_profile_enable(1) == 0
        assert p.lib.bgls_verify_aggregate_distinct(p.cid, B(agg), B(b"".join(keys)), B(b"".join(msgs)), offsets(msgs), n) == 1
        assert launches("key_msgs") >= 1 and launches("h2c") >= 1 and launches("dup_check") == 0
        assert p.lib.bgls_profile_enable(1) == 0
        pre = [k + m for k, m in zip(keys, msgs)]
        assert p.lib.bgls_verify_aggregate(p.cid, B(agg), B(b"".join(keys)), B(b"".join(pre)), offsets(pre), n, 0) == 1
        assert launches("key_msgs") == 0 and launches("dup_check") == 1
    finally:
        p.lib.bgls_profile_enable(0)
