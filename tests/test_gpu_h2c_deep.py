"""GPU tier, hash-to-G1 through the shipped library (bgls_hash_to_g1) where random messages do not reach:

  * real Keccak at try counts up to 19: the mined fixture tests/golden/h2c_deep_altbn128.json (two 64-byte messages per first accepting
    counter 0..18; 5 is the first counter of the middle schedule's <32> round, 15 of the wide kernel's second pass, 16 of the lean
    schedule's <32> round) alone (n < 256: k_h2c_bn_wide), padded to n = 300 (middle schedule) and at n = 300 in throughput mode (lean
    schedule); one deep message signed and verified;
  * every message length 0..280 on both curves, packed back to back so that the messages start at every residue mod 8 (ByteSrc::le64 does
    one unaligned 8-byte load for words inside the message, in the device build only): the single-byte 0x81 Keccak pad (length 134 after
    the prefix byte), the exact-block BLAKE2b case (124 + the 4-byte tag), two rate / block boundaries of each hash.

The schedules at ALL counters are pinned with scripted digests in test_gpu_h2c_schedule.py; this file pins the real hash in front of them."""
import ctypes
import random

import pytest

from oracle import coracle
from tests.conftest import CURVES, load_golden

pytestmark = pytest.mark.gpu


def B(b):
    return (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(bytes(b) if b else b"\0")


def offsets(msgs):
    off = (ctypes.c_uint64 * (len(msgs) + 1))()
    acc = 0
    for i, m in enumerate(msgs):
        off[i] = acc
        acc += len(m)
    off[len(msgs)] = acc
    return off


def hash_batch(lib, cid, msgs):
    """the messages packed back to back in one blob that ends with the last message's last byte"""
    fp2 = 2 * coracle.FP[cid]
    o = (ctypes.c_uint8 * (len(msgs) * fp2))()
    rc = lib.bgls_hash_to_g1(cid, B(b"".join(msgs)), offsets(msgs), len(msgs), o)
    assert rc == 0, rc
    raw = bytes(o)
    return [raw[i * fp2:(i + 1) * fp2] for i in range(len(msgs))]


# ---------------------------------------------------------------------------------------------------------------- mined messages
@pytest.fixture(scope="module")
def deep():
    return load_golden("h2c_deep_altbn128.json")["rows"]


def test_deep_messages_under_the_wide_kernel_and_both_round_schedules(gpu_lib, deep):
    lib = gpu_lib
    msgs = [bytes.fromhex(r["msg"]) for r in deep]
    want = [bytes.fromhex(r["point"]) for r in deep]
    assert {r["counter"] for r in deep} >= set(range(17)) and len(msgs) < 256
    rnd = random.Random(1919)
    pad = [rnd.randbytes(64) for _ in range(300 - len(msgs))]
    # the fixture rows spread over the batch, not in front of it
    slots = sorted(rnd.sample(range(300), len(msgs)))
    batch, it_m, it_p, taken = [], iter(msgs), iter(pad), set(slots)
    for i in range(300):
        batch.append(next(it_m) if i in taken else next(it_p))
    wide = hash_batch(lib, 0, msgs)
    middle = hash_batch(lib, 0, batch)
    try:
        assert lib.bgls_set_throughput_mode(1) == 0
        lean = hash_batch(lib, 0, batch)
    finally:
        lib.bgls_set_throughput_mode(0)
    for k, r in enumerate(deep):
        assert wide[k] == want[k], ("wide", r["counter"])
        assert middle[slots[k]] == want[k], ("middle", r["counter"])
        assert lean[slots[k]] == want[k], ("lean", r["counter"])
    assert middle == lean and [middle[s] for s in slots] == wide
    for i in range(0, 300, 37):                                   # the padding is hashed as ever
        assert middle[i] == coracle.hash_to_g1(0, batch[i])


def test_deep_message_signed_and_verified(gpu_lib, deep):
    """bgls_sign_batch and bgls_verify_aggregate hash on their own paths: a batch with the deepest messages of the fixture (and those at
    15 and 16 tries' counters) verifies, and no longer with one byte of a deep message flipped."""
    lib, fp = gpu_lib, 32
    rnd = random.Random(2020)
    by = {}
    for r in deep:
        by.setdefault(r["counter"], bytes.fromhex(r["msg"]))
    top = max(by)
    msgs = [rnd.randbytes(64), by[15], rnd.randbytes(64), by[16], by[top], rnd.randbytes(64)]
    n = len(msgs)
    sks = [rnd.randrange(1, 1 << 250) for _ in range(n)]
    kb = B(b"".join(s.to_bytes(32, "big") for s in sks))
    keys = (ctypes.c_uint8 * (n * 4 * fp))()
    assert lib.bgls_scale_generator(0, 2, kb, n, keys) == 0
    sigs = (ctypes.c_uint8 * (n * 2 * fp))()
    assert lib.bgls_sign_batch(0, kb, B(b"".join(msgs)), offsets(msgs), n, sigs) == 0
    for i in (1, 3, 4):
        assert bytes(sigs)[64 * i:64 * i + 64] == coracle.scale_point(0, 1, coracle.hash_to_g1(0, msgs[i]), sks[i])
    agg = (ctypes.c_uint8 * (2 * fp))()
    assert lib.bgls_aggregate_points(0, 1, sigs, n, agg) == 0
    assert lib.bgls_verify_aggregate(0, agg, keys, B(b"".join(msgs)), offsets(msgs), n, 0) == 1
    assert coracle.verify_aggregate(0, bytes(agg), bytes(keys), msgs, False, threads=4) == 1
    bad = list(msgs)
    bad[4] = bad[4][:40] + bytes([bad[4][40] ^ 0x10]) + bad[4][41:]
    assert lib.bgls_verify_aggregate(0, agg, keys, B(b"".join(bad)), offsets(bad), n, 0) == 0


# ---------------------------------------------------------------------------------------------------------------- lengths and alignments
LENGTHS = list(range(281))


@pytest.fixture(scope="module")
def sweep():
    """one seeded message per length 0..280 and, per curve, the C oracle's points: computed once, shared by both orders"""
    rnd = random.Random(281)
    msgs = [rnd.randbytes(n) for n in LENGTHS]
    return msgs, {cid: [coracle.hash_to_g1(cid, m) for m in msgs] for cid, _ in CURVES}


@pytest.mark.parametrize("order", ("ascending", "descending"))
@pytest.mark.parametrize("cid", [c[0] for c in CURVES], ids=[c[1] for c in CURVES])
def test_every_length_and_start_offset(gpu_lib, sweep, cid, order):
    msgs, want = sweep[0], sweep[1][cid]
    idx = list(range(len(msgs))) if order == "ascending" else list(range(len(msgs) - 1, -1, -1))
    lens = [len(msgs[i]) for i in idx]
    assert sorted(lens) == LENGTHS and {123, 124, 125, 134, 135, 136, 251, 252, 253, 270, 271, 272} <= set(lens)
    starts = [sum(lens[:k]) for k in range(len(lens))]
    # every residue mod 8 as a start offset, among the messages long enough to have a word inside them
    assert {s % 8 for s, n in zip(starts, lens) if n >= 16} == set(range(8))
    got = hash_batch(gpu_lib, cid, [msgs[i] for i in idx])          # 281: the round kernels (alt-bn128) / the staged kernels
    for i, g in zip(idx, got):
        assert g == want[i], ("batch of 281", len(msgs[i]))
    for part in (idx[:141], idx[141:]):                             # n < 256: the wide kernel on alt-bn128
        sub = [len(msgs[i]) for i in part]
        assert {sum(sub[:k]) % 8 for k in range(len(sub)) if sub[k] >= 16} == set(range(8))
        got = hash_batch(gpu_lib, cid, [msgs[i] for i in part])
        for i, g in zip(part, got):
            assert g == want[i], ("batch of %d" % len(part), len(msgs[i]))
