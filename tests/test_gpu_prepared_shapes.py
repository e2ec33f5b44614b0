"""GPU tier: the prepared-key fold (BGLS_KEYS_PREPARE: k_prepare, k_prep_points, k_fold_prep of bgls_amd/csrc/prepared.hpp) at every
group size, wave seam, chunk seam and degenerate key.

The fold's shape is chosen at upload: ng pairings per accumulator group and squaring (6 below 60 x 2 816 / 2 048 keys per shard, up to 96
above), the set padded to whole waves of 10 ng pairings, the keys prepared 2^17 per launch.  bgls_set_prepare_shape(ng, chunk) forces
both, so that the m loop with its two-slot line ring, the prefetch that crosses from m = ng - 1 into the next step, the skip word, the
padding and the per-chunk scratch of k_prepare are all reached with a few hundred keys.

The comparison value throughout is the GT element of bgls_verify_aggregate_h_gt under a WRONG signature (a signer's who is not in the
set): a generic element of GT, whose bytes change with any dropped, repeated or misplaced line.  The reference is the same call on the
unprepared upload of the same keys (pinned to the C oracle in test_gpu_x60.py and test_gpu_keys.py) and, at the smallest size of each
group size and wherever stated, the oracle's pairing product itself.  Every comparison is byte for byte.

Every test leaves bgls_set_prepare_shape(0, 0) in force and frees every key set, pass or fail (the two autouse fixtures below)."""
import ctypes

import pytest

from oracle import coracle
from tests.conftest import load_golden
from test_gpu_keys import B, ORDER, devs, make_instance, offsets, out

pytestmark = pytest.mark.gpu

CHECK, PREPARE = 1, 2                      # BGLS_KEYS_CHECK, BGLS_KEYS_PREPARE
ERR_ARG, ERR_ENCODING = -1, -2
NGS = (6, 7, 13, 38, 52, 96)
# one key; one full group; one key into the second group; both sides of a wave seam; a third wave that holds a single real key
SIZES = {"one": lambda ng: 1, "group": lambda ng: ng, "group+1": lambda ng: ng + 1, "wave-1": lambda ng: 10 * ng - 1,
         "wave": lambda ng: 10 * ng, "wave+1": lambda ng: 10 * ng + 1, "2waves+1": lambda ng: 20 * ng + 1}
POOL = 20 * max(NGS) + 2                   # the largest set and one signer who is in none of them

_pools = {}
_ref_gts = {}


def pool(lib, curve):
    """POOL signers of one curve, made once: every set below is a prefix of it (reference values are shared and never changed)"""
    cid = curve["id"]
    if cid not in _pools:
        sks, keys, msgs, sigs, _ = make_instance(lib, cid, curve["fp"], POOL, 9100 + cid)
        _pools[cid] = {"sks": sks, "keys": keys, "msgs": msgs, "sigs": sigs}
    return _pools[cid]


def prefix(lib, curve, n):
    """keys, messages and aggregate of the first n signers; `wrong`: the signature of the pool's last signer, who is in no set"""
    cid, fp = curve["id"], curve["fp"]
    p = pool(lib, curve)
    assert n < POOL
    agg = out(2 * fp)
    assert lib.bgls_aggregate_points(cid, 1, B(p["sigs"][:2 * fp * n]), n, agg) == 0
    return {"n": n, "keys": p["keys"][:4 * fp * n], "msgs": p["msgs"][:n], "sigs": p["sigs"][:2 * fp * n], "agg": bytes(agg),
            "wrong": p["sigs"][2 * fp * (POOL - 1):]}


def flipped(msgs, at):
    bad = list(msgs)
    bad[at] = bytes([bad[at][0] ^ 1]) + bad[at][1:]
    return bad


def last_error():
    from bgls_amd import _lib
    return _lib.last_error()


class KeySets:
    """uploads that are freed when the test ends, whatever became of it"""

    def __init__(self, lib, curve):
        self.lib, self.cid, self.fp, self.open = lib, curve["id"], curve["fp"], []

    def upload(self, keys, n, flags, shards=1):
        h = ctypes.c_uint64()
        rc = self.lib.bgls_keys_upload(self.cid, B(keys), n, devs(shards), shards, flags, ctypes.byref(h))
        assert rc == 0, (rc, last_error())
        self.open.append(h.value)
        return h

    def free(self, h):
        assert self.lib.bgls_keys_free(h) == 0
        self.open.remove(h.value)

    def free_all(self):
        left, self.open = self.open, []
        return [self.lib.bgls_keys_free(ctypes.c_uint64(v)) for v in left]

    def verdict(self, h, sig, msgs):
        return self.lib.bgls_verify_aggregate_h(h, B(sig), B(b"".join(msgs)), offsets(msgs), len(msgs), 0)

    def gt(self, h, sig, msgs):
        g = out(12 * self.fp)
        rc = self.lib.bgls_verify_aggregate_h_gt(h, B(sig), B(b"".join(msgs)), offsets(msgs), len(msgs), 0, g)
        assert rc in (0, 1), (rc, last_error())
        return bytes(g)

    def unprepared_gt(self, keys, n, sig, msgs, shards=1):
        h = self.upload(keys, n, 0, shards)
        g = self.gt(h, sig, msgs)
        self.free(h)
        return g


@pytest.fixture(autouse=True)
def _automatic_shape_afterwards(gpu_lib):
    yield
    assert gpu_lib.bgls_set_prepare_shape(0, 0) == 0


@pytest.fixture
def sets(gpu_lib, curve):
    ks = KeySets(gpu_lib, curve)
    yield ks
    assert all(rc == 0 for rc in ks.free_all())


def shape(lib, ng, chunk=0):
    assert lib.bgls_set_prepare_shape(ng, chunk) == 0


def ref_gt(sets, curve, inst):
    """the unprepared set's GT bytes for a prefix of the pool under the wrong signature, computed once per size"""
    key = (curve["id"], inst["n"])
    if key not in _ref_gts:
        _ref_gts[key] = sets.unprepared_gt(inst["keys"], inst["n"], inst["wrong"], inst["msgs"])
    return _ref_gts[key]


def oracle_gt(lib, curve, keys, msgs, wrong):
    """prod e(H(m_i), pk_i) * e(-wrong, g2) by the C oracle"""
    cid, fp = curve["id"], curve["fp"]
    g2 = out(4 * fp)
    assert lib.bgls_generator(cid, 2, g2) == 0
    g1s = b"".join(coracle.hash_to_g1(cid, m) for m in msgs) + coracle.scale_point(cid, 1, wrong, ORDER[cid] - 1)
    return coracle.pairing_product(cid, g1s, bytes(keys) + bytes(g2), len(msgs) + 1, threads=8)


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("ng", NGS)
def test_every_group_size_at_group_and_wave_seams(gpu_lib, curve, sets, ng, size):
    """ng in 6, 7, 13, 38, 52, 96 (the automatic rule reaches 6 below 1.2e5 keys and 38 / 52 at 2^20 only), n on both sides of every
    seam of the fold: the wrong-signature GT equals the unprepared set's bytes (at n = 1 also the oracle's), the valid aggregate is
    accepted, a message flipped at the last position and at the last slot of the first group is refused."""
    lib, n = gpu_lib, SIZES[size](ng)
    inst = prefix(lib, curve, n)
    want = ref_gt(sets, curve, inst)
    assert want != bytes(12 * curve["fp"] - 1) + b"\x01"
    shape(lib, ng)
    h = sets.upload(inst["keys"], n, CHECK | PREPARE)
    shape(lib, 0)                                          # a resident set keeps the shape it was uploaded with
    assert sets.gt(h, inst["wrong"], inst["msgs"]) == want, (ng, n)
    if size == "one":
        assert want == oracle_gt(lib, curve, inst["keys"], inst["msgs"], inst["wrong"]), ng
    assert sets.verdict(h, inst["agg"], inst["msgs"]) == 1, (ng, n)
    assert sets.verdict(h, inst["agg"], flipped(inst["msgs"], n - 1)) == 0, (ng, n)
    if ng - 1 < n - 1:
        assert sets.verdict(h, inst["agg"], flipped(inst["msgs"], ng - 1)) == 0, (ng, n)
    sets.free(h)


def test_the_automatic_rule_is_the_default(gpu_lib, curve, sets):
    """with the knob at (0, 0) a 333-key set (prep_ng: 6) gives the bytes of the set forced to ng = 6, which are the unprepared set's"""
    lib = gpu_lib
    inst = prefix(lib, curve, 333)
    got = []
    for ng in (0, 6):
        shape(lib, ng)
        h = sets.upload(inst["keys"], 333, PREPARE)
        got.append(sets.gt(h, inst["wrong"], inst["msgs"]))
        sets.free(h)
    assert got[0] == got[1] == ref_gt(sets, curve, inst)


@pytest.mark.parametrize("ng,chunk,n", [(6, c, n) for c in (1, 59, 64, 100) for n in (61, 130)] + [(13, 64, 131)])
def test_chunk_seams_of_the_preparation(gpu_lib, curve, sets, ng, chunk, n):
    """k_prepare in chunks of 1, 59, 64 and 100 keys over n_pad = 120 / 180 (ng = 6) and 260 (ng = 13): seams inside a wave, inside a
    group and between real keys and padding, a last chunk shorter than the others (its scratch is indexed by its own count).  Same
    bytes as the one-chunk upload of the same keys and as the unprepared set."""
    lib = gpu_lib
    inst = prefix(lib, curve, n)
    got = []
    for c in (0, chunk):
        shape(lib, ng, c)
        h = sets.upload(inst["keys"], n, PREPARE)
        got.append(sets.gt(h, inst["wrong"], inst["msgs"]))
        if c:
            assert sets.verdict(h, inst["agg"], inst["msgs"]) == 1
            assert sets.verdict(h, inst["agg"], flipped(inst["msgs"], n - 1)) == 0
        sets.free(h)
    assert got[1] == got[0], (ng, chunk, n)
    assert got[0] == ref_gt(sets, curve, inst)


INF_AT = (0, 6, 7, 69, 70, 139, 140)


@pytest.mark.parametrize("ng,shards", [(7, 1), (6, 3)])
def test_keys_at_infinity_at_every_seam(gpu_lib, curve, sets, ng, shards):
    """141 keys at ng = 7 (n_pad = 210), keys at infinity in the first slot, the last slot of a group and the first of the next
    (6, 7), the two sides of the wave seam (69, 70), and the last two real keys in front of the padding (139, 140); again at ng = 6 on
    three shards of 47 keys, each with a padding of its own.  e(H, infinity) = 1: the aggregate without those signers is accepted,
    the full aggregate refused, and the wrong-signature GT is the unprepared set's and the oracle's over the remaining pairs."""
    lib, cid, fp, n = gpu_lib, curve["id"], curve["fp"], 141
    inst = prefix(lib, curve, n)
    keys = bytearray(inst["keys"])
    for i in INF_AT:
        keys[4 * fp * i:4 * fp * (i + 1)] = bytes(4 * fp)
    keys = bytes(keys)
    rest = [i for i in range(n) if i not in INF_AT]
    agg = out(2 * fp)
    assert lib.bgls_aggregate_points(cid, 1, B(b"".join(inst["sigs"][2 * fp * i:2 * fp * (i + 1)] for i in rest)), len(rest), agg) == 0
    want = sets.unprepared_gt(keys, n, inst["wrong"], inst["msgs"], shards)
    shape(lib, ng)
    h = sets.upload(keys, n, PREPARE, shards)
    assert sets.verdict(h, bytes(agg), inst["msgs"]) == 1
    assert sets.verdict(h, inst["agg"], inst["msgs"]) == 0
    assert sets.gt(h, inst["wrong"], inst["msgs"]) == want
    sets.free(h)
    live_keys = b"".join(keys[4 * fp * i:4 * fp * (i + 1)] for i in rest)
    assert want == oracle_gt(lib, curve, live_keys, [inst["msgs"][i] for i in rest], inst["wrong"])


@pytest.mark.parametrize("ng", (0, 7))
def test_a_shard_without_keys_is_all_padding(gpu_lib, curve, sets, ng):
    """two keys on three shards: the first shard holds no key (its prepared table is one wave of padding, and it is the shard that
    pairs the signature), the others one key each behind 10 ng - 1 padding entries"""
    lib = gpu_lib
    inst = prefix(lib, curve, 2)
    shape(lib, ng)
    h = sets.upload(inst["keys"], 2, CHECK | PREPARE, 3)
    assert sets.gt(h, inst["wrong"], inst["msgs"]) == ref_gt(sets, curve, inst)
    assert sets.verdict(h, inst["agg"], inst["msgs"]) == 1
    assert sets.verdict(h, inst["agg"], flipped(inst["msgs"], 0)) == 0
    sets.free(h)


def off_subgroup_rows(curve):
    rows = [r for r in load_golden("subgroup_%s.json" % curve["name"])["points"] if r["on_twist"] and not r["in_subgroup"]]
    return [r for r in rows if not r["miller_degenerates"]], [r for r in rows if r["miller_degenerates"]]


def test_twist_points_outside_g2_as_prepared_keys(gpu_lib, curve, sets):
    """Twist points outside the order-r subgroup whose point steps do not degenerate, uploaded without BGLS_KEYS_CHECK, one between
    every two valid keys: the prepared upload succeeds and the wrong-signature GT equals the unprepared set's bytes.  On alt-bn128
    it also equals the oracle's pairing product.  On BLS12-381 it is NOT compared with the oracle: the engine pairs the uncleared
    hash points and raises the product to the G1 cofactor in GT, which for a key outside G2 is another function of the inputs than
    the oracle's product over cleared hash points."""
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    plain, _ = off_subgroup_rows(curve)
    assert len(plain) >= 1
    n = 2 * len(plain) + 1
    inst = prefix(lib, curve, n)
    keys = bytearray(inst["keys"])
    for j, r in enumerate(plain):
        keys[4 * fp * (2 * j + 1):4 * fp * (2 * j + 2)] = bytes.fromhex(r["pt"])
    keys = bytes(keys)
    want = sets.unprepared_gt(keys, n, inst["wrong"], inst["msgs"])
    for ng in (6, 7):
        shape(lib, ng)
        h = sets.upload(keys, n, PREPARE)
        assert sets.gt(h, inst["wrong"], inst["msgs"]) == want, ng
        sets.free(h)
    if cid == 0:
        assert want == oracle_gt(lib, curve, keys, inst["msgs"], inst["wrong"])


def test_a_key_with_a_degenerate_step_cannot_be_prepared(gpu_lib, curve, sets):
    """BLS12-381's twist point of order 13 (T = +-Q after six steps: c2 = 0) among 20 valid keys, first, in the middle and last: the
    prepared upload is refused with BGLS_ERR_ENCODING and writes no handle; unprepared the same keys upload, with the subgroup check
    they fail on that check; the next prepared upload of valid keys succeeds and verifies (the flag word was reset).  alt-bn128's
    twist has no such point (its smallest cofactor order is 10069), which is all this test states there."""
    lib, cid, fp, n = gpu_lib, curve["id"], curve["fp"], 20
    _, deg = off_subgroup_rows(curve)
    assert len(deg) == (1 if cid == 1 else 0)
    inst = prefix(lib, curve, n)
    want = ref_gt(sets, curve, inst)
    for r in deg:
        for at in (0, 9, 19):
            keys = bytearray(inst["keys"])
            keys[4 * fp * at:4 * fp * (at + 1)] = bytes.fromhex(r["pt"])
            keys = bytes(keys)
            h = ctypes.c_uint64(0xDEAD)
            assert lib.bgls_keys_upload(cid, B(keys), n, devs(1), 1, PREPARE, ctypes.byref(h)) == ERR_ENCODING, at
            assert "cannot be prepared" in last_error() and h.value == 0xDEAD, at
            sets.free(sets.upload(keys, n, 0))
            assert lib.bgls_keys_upload(cid, B(keys), n, devs(1), 1, CHECK | PREPARE, ctypes.byref(h)) == ERR_ENCODING, at
            assert "subgroup" in last_error() and h.value == 0xDEAD, at
            good = sets.upload(inst["keys"], n, PREPARE)
            assert sets.verdict(good, inst["agg"], inst["msgs"]) == 1, at
            assert sets.gt(good, inst["wrong"], inst["msgs"]) == want, at
            sets.free(good)


def miller_partial(lib, curve, h, t_sig, msgs):
    """the prepared set's Miller product BEFORE the final exponentiation (bgls_miller_product_keys_dev), messages of 64 bytes"""
    import torch
    gtb = 12 * curve["fp"]
    t_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to("cuda:0")
    part = torch.zeros(gtb, dtype=torch.uint8, device="cuda:0")
    flags = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rc = lib.bgls_miller_product_keys_dev(h, t_sig.data_ptr(), t_msgs.data_ptr(), 64, 64, len(msgs), 0, part.data_ptr(), flags.data_ptr(), None)
    assert rc == 0, (rc, last_error())
    torch.cuda.synchronize()
    assert int(flags[0]) == 0
    return bytes(part.cpu().numpy())


def test_a_skipped_line_is_exactly_one_before_the_final_exponentiation(gpu_lib, curve, sets):
    """The final exponentiation hides a wrong factor from a proper subfield of Fp12, and the line of an all-zero table entry is
    such a factor (w^3 on the D-type twist, 1 on the M-type): a fold that ignores the skip word of a padding entry or of a key at
    infinity still lands on the right GT bytes.  The Miller product itself does not forgive it.  It is one field element whatever
    the grouping, so (1) the partial of the same 61 / 141 keys is the same bytes at every ng -- the count of groups whose last slot
    is padding differs between them -- and (2) the 141-key set with seven keys at infinity (three of them in the last slot of a
    group at ng = 7) gives the bytes of the 134-key set without those keys and messages."""
    import random
    import torch
    lib, cid, fp = gpu_lib, curve["id"], curve["fp"]
    p = pool(lib, curve)
    rnd = random.Random(515 + cid)
    msgs = [rnd.randbytes(64) for _ in range(141)]
    t_sig = torch.frombuffer(bytearray(p["sigs"][:2 * fp]), dtype=torch.uint8).to("cuda:0")

    def partial(keys, ms, ng, chunk=0):
        shape(lib, ng, chunk)
        h = sets.upload(keys, len(ms), PREPARE)
        got = miller_partial(lib, curve, h, t_sig, ms)
        sets.free(h)
        return got

    for n in (61, 141):
        keys = p["keys"][:4 * fp * n]
        want = partial(keys, msgs[:n], 0)
        for ng in NGS:
            assert partial(keys, msgs[:n], ng) == want, (n, ng)
        assert partial(keys, msgs[:n], 7, 59) == want, n
    rest = [i for i in range(141) if i not in INF_AT]
    holes = bytearray(p["keys"][:4 * fp * 141])
    for i in INF_AT:
        holes[4 * fp * i:4 * fp * (i + 1)] = bytes(4 * fp)
    live_keys = b"".join(p["keys"][4 * fp * i:4 * fp * (i + 1)] for i in rest)
    want = partial(live_keys, [msgs[i] for i in rest], 0)
    for ng in (6, 7, 13):
        assert partial(bytes(holes), msgs, ng) == want, ng
        assert partial(live_keys, [msgs[i] for i in rest], ng) == want, ng


def test_forced_shape_behind_poisoned_and_larger_workspaces(gpu_lib, curve, sets):
    """WS_LINES is sized by n_pad, which the shape moves: 131 keys at ng = 13 give the same bytes on a fresh call, behind
    bgls_selftest_fill_workspaces(0xFF) (the resident ratios are not a workspace and survive it) and behind a larger prepared call at
    ng = 38 over 400 keys."""
    lib = gpu_lib
    small, big = prefix(lib, curve, 131), prefix(lib, curve, 400)
    shape(lib, 13)
    h = sets.upload(small["keys"], 131, PREPARE)
    shape(lib, 38)
    hb = sets.upload(big["keys"], 400, PREPARE)
    want = ref_gt(sets, curve, small)
    assert sets.gt(h, small["wrong"], small["msgs"]) == want
    filled = ctypes.c_uint64(0)
    assert lib.bgls_selftest_fill_workspaces(0xFF, h, ctypes.byref(filled)) == 0 and filled.value > 0
    assert sets.gt(h, small["wrong"], small["msgs"]) == want
    assert lib.bgls_selftest_fill_workspaces(0xFF, h, ctypes.byref(filled)) == 0
    assert sets.verdict(h, small["agg"], small["msgs"]) == 1
    assert sets.gt(hb, big["wrong"], big["msgs"]) == ref_gt(sets, curve, big)
    assert sets.gt(h, small["wrong"], small["msgs"]) == want
    assert sets.verdict(h, small["agg"], flipped(small["msgs"], 130)) == 0
    sets.free(h)
    sets.free(hb)


def test_a_rejected_setting_changes_nothing(gpu_lib, curve, sets):
    """(97, 0) and (5, 0) behind (7, 0) are refused and the next upload still verifies with the reference's bytes.  That it was
    prepared at 7 and not at the automatic 6 is not observable through the ABI (n_pad shows only in the capacity of cached workspaces,
    which earlier tests of a session have already grown), so this states the refusal and the unbroken state alone."""
    lib = gpu_lib
    inst = prefix(lib, curve, 61)
    shape(lib, 7)
    assert lib.bgls_set_prepare_shape(97, 0) == ERR_ARG and "ng" in last_error()
    assert lib.bgls_set_prepare_shape(5, 0) == ERR_ARG
    h = sets.upload(inst["keys"], 61, PREPARE)
    assert sets.gt(h, inst["wrong"], inst["msgs"]) == ref_gt(sets, curve, inst)
    assert sets.verdict(h, inst["agg"], inst["msgs"]) == 1
    sets.free(h)
